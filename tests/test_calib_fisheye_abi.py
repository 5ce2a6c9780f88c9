"""The fisheye calibration's share of the C ABI: include/aprilslam.h declares asl_calibrate_lens_frames_device /
asl_calibrate_lens_batch in the argument order of asl_calibrate_*, lens_model before n_dist; the library exports them; the
result record is asl_calib_result's 216 bytes; and the entry points refuse a NULL detector before they touch a device or an
output.  (The refusals that need a detector are in test_gpu_calibrate_fisheye.py.)  No GPU."""
import ctypes as C
import inspect

import numpy as np

import test_abi
from aprilslam_amd import _lib
from test_smooth_cov_abi import prototype

NAMES = ["asl_calibrate_lens_frames_device", "asl_calibrate_lens_batch"]


def test_entry_points_are_declared_listed_and_exported():
    declared = test_abi.declared_functions()
    L = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
    assert L.asl_calibrate_lens_frames_device.argtypes[:-1] == L.asl_calibrate_lens_batch.argtypes
    assert len(L.asl_calibrate_lens_batch.argtypes) == 16 == len(prototype("asl_calibrate_lens_batch"))


def test_the_argument_order_is_the_brown_calls_with_the_lens_before_n_dist():
    for old, new in (("asl_calibrate_frames_device", NAMES[0]), ("asl_calibrate_batch", NAMES[1])):
        po, pn = prototype(old), prototype(new)
        k = pn.index("lens_model")
        assert pn[k + 1] == "n_dist" and pn[k - 1] == "K_init" and pn[:k] + pn[k + 1:] == po, (po, pn)
        L = _lib.load()
        a = getattr(L, new).argtypes
        assert a[k] == C.c_int and list(a[:k]) + list(a[k + 1:]) == list(getattr(L, old).argtypes)


def test_the_record_is_the_brown_calls_216_bytes():
    assert _lib.CALIB_RESULT_DTYPE.itemsize == 216
    assert _lib.CALIB_RESULT_DTYPE.fields["dist"][0].shape == (5,) and _lib.CALIB_RESULT_DTYPE.fields["std"][0].shape == (9,)
    assert (_lib.LENS_BROWN, _lib.LENS_FISHEYE) == (0, 1)


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.zeros((2, 4), dtype=_lib.OBS_DTYPE)
    rec = np.zeros(4, dtype=_lib.MAP_TAG_DTYPE)
    res = np.full(216, 0xAB, dtype=np.uint8)
    poses = np.full(2 * _lib.CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    args = (obs.ctypes.data, 2, 4, rec.ctypes.data, 4, 10.0, 640, 480, None, 1, 4, 0, 5, res.ctypes.data, poses.ctypes.data)
    assert L.asl_calibrate_lens_batch(None, *args) == -1
    assert b"detector" in L.asl_last_error()
    assert L.asl_calibrate_lens_frames_device(None, *args, None) == -1
    assert b"detector" in L.asl_last_error()
    assert (res == 0xAB).all() and (poses == 0xAB).all()


def test_python_surface():
    import pytest

    from aprilslam_amd.calibrate import CalibrationResult
    from aprilslam_amd.tag_detector import TagDetector
    for f in (_lib.Detector.calibrate, _lib.Detector.calibrate_device):
        assert inspect.signature(f).parameters["model"].default is None
    assert inspect.signature(TagDetector.calibrate).parameters["lens_model"].default == "brown"
    assert inspect.signature(CalibrationResult.__init__).parameters["lens_model"].default == "brown"
    assert callable(CalibrationResult.view_set)
    # what the Python layer refuses before it reaches the library
    with pytest.raises(ValueError):
        _lib.Detector._calib_args(None, 5, "fisheye")
    with pytest.raises(ValueError):
        _lib.Detector._calib_args(None, 4, "pinhole")
    assert _lib.Detector._calib_args(None, 4, "fisheye")[2] == 1 and _lib.Detector._calib_args(None, 5, "brown")[2] == 0
    assert _lib.Detector._calib_args(None, 5)[2] is None
