"""The ABI of the sequence localisation with frame times: include/aprilslam.h declares asl_smooth_timed_sequences_device / _batch as
the robust several-sequences argument lists with the times after the seed, the library exports them, the ctypes argument
lists agree, the Python surface has the `times` keywords, the host entry point refuses a NULL detector before it touches a
device, and SmoothResult.pose_at is the statement's.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import smooth_cases as SC
import smooth_ref as SR
import smooth_timed_cases as TC
from aprilslam_amd import _lib
from aprilslam_amd.smooth import STATUS_BAD_TIMES, SmoothResult
from test_smooth_cov_abi import ROOT, prototype


def test_header_prototypes():
    for form, new, count in (("device", "d_times", 23), ("batch", "times", 22)):
        rob, timed = prototype("asl_smooth_robust_sequences_" + form), prototype("asl_smooth_timed_sequences_" + form)
        at = rob.index("d_seed" if form == "device" else "seed") + 1
        want = rob[:at] + [new] + rob[at:]
        want[want.index("huber_px")] = "huber"
        assert timed == want and len(timed) == count and timed[at + 1] == "seq_start"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aprilslam.h")).read(), flags=re.S)
    assert len(re.findall(r"const\s+double\s*\*\s*d_times", src)) == 1 and len(re.findall(r"const\s+double\s*\*\s*times", src)) == 1
    assert len(re.findall(r"double\s+huber\s*,", src)) == 2
    body = re.search(r"typedef struct \{([^}]*)\}\s*asl_smooth_result;", open(os.path.join(ROOT, "include", "aprilslam.h")).read(), flags=re.S).group(1)
    assert re.search(r"\b4 \(asl_smooth_timed_sequences_\*\)", body)      # the new status is documented in the struct comment


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_smooth_timed_sequences_device", "asl_smooth_timed_sequences_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    dev, host = L.asl_smooth_robust_sequences_device.argtypes, L.asl_smooth_robust_sequences_batch.argtypes
    assert L.asl_smooth_timed_sequences_device.argtypes == dev[:11] + [C.c_void_p] + dev[11:]
    assert L.asl_smooth_timed_sequences_batch.argtypes == host[:11] + [C.POINTER(C.c_double)] + host[11:]
    assert len(L.asl_smooth_timed_sequences_device.argtypes) == len(prototype("asl_smooth_timed_sequences_device")) == 23
    assert len(L.asl_smooth_timed_sequences_batch.argtypes) == len(prototype("asl_smooth_timed_sequences_batch")) == 22
    assert _lib.SMOOTH_RESULT_DTYPE.itemsize == 64 and STATUS_BAD_TIMES == SR.BAD_TIMES == 4


def test_python_surface_has_the_argument():
    from aprilslam_amd.tag_detector import TagDetector
    for fn in (_lib.Detector.smooth, _lib.Detector.smooth_sequences, TagDetector.localize_sequence):
        assert inspect.signature(fn).parameters["times"].default is None, fn
    for fn in (_lib.Detector.smooth_device, _lib.Detector.smooth_sequences_device):
        assert inspect.signature(fn).parameters["times_ptr"].default is None, fn
    p = list(inspect.signature(SmoothResult.__init__).parameters)
    assert p[-1] == "times" and inspect.signature(SmoothResult.__init__).parameters["times"].default is None


def test_null_detector_is_refused():
    L = _lib.load()
    b, times = TC.bad_times_batch()
    n, mt = b.obs.shape
    n_seq = len(b.seq_start) - 1
    obs, seed, Kc = np.ascontiguousarray(b.obs), np.ascontiguousarray(b.seed), np.ascontiguousarray(SC.K)
    tm = np.ascontiguousarray(times)
    out = np.full(n * _lib.CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    res = np.full(n_seq * 64, 0xAB, dtype=np.uint8)
    cov = np.full(n * _lib.POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    start = np.ascontiguousarray(b.seq_start, dtype=np.int32)
    DP = C.POINTER(C.c_double)
    rc = L.asl_smooth_timed_sequences_batch(None, obs.ctypes.data, n, mt, b.rec.ctypes.data, len(b.rec), Kc.ctypes.data_as(DP), None, 0, SC.TAG,
                                            seed.ctypes.data, tm.ctypes.data_as(DP), start.ctypes.data_as(C.POINTER(C.c_int32)), n_seq, *b.sigmas,
                                            0.0, b.max_iters, out.ctypes.data, res.ctypes.data, cov.ctypes.data)
    assert rc == -1 and b"detector" in L.asl_last_error()
    assert (out == 0xAB).all() and (res == 0xAB).all() and (cov == 0xAB).all()
    rc = L.asl_smooth_timed_sequences_device(None, 256, n, mt, 256, len(b.rec), Kc.ctypes.data_as(DP), None, 0, SC.TAG, 256, 256,
                                             start.ctypes.data_as(C.POINTER(C.c_int32)), n_seq, *b.sigmas, 0.0, b.max_iters, 256, 256, None, None)
    assert rc == -1 and b"detector" in L.asl_last_error()


def hand_made(n=4):
    """n poses on a gentle arc, world<-camera"""
    poses = np.zeros(n, dtype=_lib.CAM_POSE_DTYPE)
    import localize_ref as LR
    for f in range(n):
        T = np.eye(4)
        T[:3, :3] = LR.rodrigues(np.array([0.02 * f, -0.05 * f, 0.03 * f * f]))
        T[:3, 3] = [0.3 * f, 0.1 * f * f, -0.2 * f]
        poses["T"][f] = T
    return poses, np.zeros((), dtype=_lib.SMOOTH_RESULT_DTYPE)


def test_pose_at_on_hand_made_records():
    poses, result = hand_made()
    times = np.array([0.0, 0.5, 2.5, 3.0])
    r = SmoothResult(poses, result, times=times)
    assert r.ok and np.array_equal(r.times, times)
    for f, t in enumerate(times):
        assert np.array_equal(r.pose_at(t), poses["T"][f])
    for t in (0.25, 0.6, 1.5, 2.49, 2.75):
        got, want = r.pose_at(t), SR.pose_at(poses["T"], times, t)
        assert np.abs(got - want).max() <= 1e-14, t
        assert np.allclose(got[:3, :3] @ got[:3, :3].T, np.eye(3), atol=1e-14) and np.array_equal(got[3], [0, 0, 0, 1])
    # the geodesic: half way in time is half the step's rotation and, camera<-world, half its translation
    mid = r.pose_at(1.5)
    Ra, Rb, Rm = poses["T"][1][:3, :3].T, poses["T"][2][:3, :3].T, mid[:3, :3].T
    assert np.allclose(SR.log_so3(Rm @ Ra.T), 0.5 * SR.log_so3(Rb @ Ra.T), atol=1e-14)
    for t in (-1e-9, 3.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            r.pose_at(t)
    # without times the frame index is the time
    plain = SmoothResult(poses, result)
    assert plain.times is None and np.array_equal(plain.pose_at(2), poses["T"][2])
    assert np.abs(plain.pose_at(1.25) - SR.pose_at(poses["T"], None, 1.25)).max() <= 1e-14
    with pytest.raises(ValueError):
        plain.pose_at(3.5)
    one = SmoothResult(poses[:1], result, times=[7.0])
    assert np.array_equal(one.pose_at(7.0), poses["T"][0])
    with pytest.raises(ValueError):
        one.pose_at(7.5)
    with pytest.raises(ValueError):
        SmoothResult(poses, result, times=times[:3])
    bad = result.copy()
    bad["status"] = STATUS_BAD_TIMES
    failed = SmoothResult(poses, bad, times=times)
    assert not failed.ok
    with pytest.raises(ValueError):
        failed.pose_at(1.0)


def test_batches_are_what_the_issue_says():
    b, times = TC.bad_times_batch()
    assert np.diff(b.seq_start).tolist() == [5, 5, 5, 5] and TC.BAD_STATUS == [0, 4, 4, 4]
    t = times.reshape(4, 5)
    assert np.isfinite(t[0]).all() and (np.diff(t[0]) > 0).all()
    assert np.isnan(t[1]).sum() == 1 and (np.diff(t[2]) == 0).sum() == 1 and (np.diff(t[3]) < 0).sum() == 1
    rb, rt = TC.ragged()
    assert np.diff(rb.seq_start).tolist() == [1, 2, 3, 5, 64, 65, 130]
    names = [c[0] for c in TC.all_cases()]
    assert names == [c[0] for c in SC.all_cases()][4:] and len(names) == len(SC.SHAPES) + 5
    for c in TC.all_cases():
        d = np.diff(c[5])
        assert len(c[5]) == len(c[1]) and (d >= 0.25).all() and (d <= 4.0).all()
