"""The rig mounting calibration's share of the C ABI: the result record's layout and the two entry points."""
import numpy as np

import test_abi
from aprilslam_amd import _lib

NAMES = ["asl_calibrate_rig_frames_device", "asl_calibrate_rig_batch"]


def test_result_record_has_the_header_layout():
    dt = _lib.RIG_CALIB_RESULT_DTYPE
    assert dt.itemsize == 176 == 3 * 8 + 6 * 4 + 16 * 4 + 16 * 4
    c = np.dtype(dt.descr, align=True)
    assert c.itemsize == dt.itemsize and [c.fields[f][1] for f in c.names] == [dt.fields[f][1] for f in dt.names]
    assert dt.names == ("rms_px", "rms_init_px", "sigma_px", "n_frames_used", "n_corners", "iterations", "status", "n_solved", "reserved",
                        "cam_status", "cam_frames")
    assert dt.fields["cam_status"][1] == 48 and dt.fields["cam_frames"][1] == 112


def test_entry_points_are_declared_listed_and_exported():
    declared = test_abi.declared_functions()
    L = _lib.load()
    for n in NAMES:
        assert n in declared and n in _lib.EXPORTS and hasattr(L, n), n
    # both take the same arguments but for the stream
    assert L.asl_calibrate_rig_frames_device.argtypes[:-1] == L.asl_calibrate_rig_batch.argtypes
    assert len(L.asl_calibrate_rig_batch.argtypes) == 15
