"""The ABI of the robust sequence localisation: include/aprilslam.h declares asl_smooth_robust_sequences_device / _batch as the
several-sequences argument lists with `huber_px` after sigma_trans, the library exports them, the ctypes argument lists
agree, asl_smooth_result carries n_soft in the first of its reserved ints, and the host entry point refuses a NULL detector
before it touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import smooth_cases as SC
import smooth_robust_cases as RC
from aprilslam_amd import _lib
from test_smooth_cov_abi import ROOT, prototype


def test_header_prototypes():
    for form in ("device", "batch"):
        seq, rob = prototype("asl_smooth_sequences_" + form), prototype("asl_smooth_robust_sequences_" + form)
        at = seq.index("sigma_trans") + 1
        assert rob == seq[:at] + ["huber_px"] + seq[at:] and rob[at + 1] == "max_iters"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aprilslam.h")).read(), flags=re.S)
    assert len(re.findall(r"double\s+huber_px", src)) == 2


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_smooth_robust_sequences_device", "asl_smooth_robust_sequences_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    dev, host = L.asl_smooth_sequences_device.argtypes, L.asl_smooth_sequences_batch.argtypes
    assert dev[13:16] == [C.c_double] * 3 and dev[16] == C.c_int
    assert L.asl_smooth_robust_sequences_device.argtypes == dev[:16] + [C.c_double] + dev[16:]
    assert L.asl_smooth_robust_sequences_batch.argtypes == host[:16] + [C.c_double] + host[16:]
    assert len(L.asl_smooth_robust_sequences_device.argtypes) == len(prototype("asl_smooth_robust_sequences_device")) == 22
    assert len(L.asl_smooth_robust_sequences_batch.argtypes) == len(prototype("asl_smooth_robust_sequences_batch")) == 21


def test_record_layout():
    dt = _lib.SMOOTH_RESULT_DTYPE
    assert dt.itemsize == 64 and dt.names[-3:] == ("status", "n_soft", "reserved")
    assert dt.fields["n_soft"][1] == 52 and dt.fields["reserved"][1] == 56 and dt.fields["reserved"][0].shape == (2,)
    assert dt.fields["status"][1] == 48 and dt.fields["n_soft"][0] == np.dtype("<i4")
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*asl_smooth_result;\s*/\*\s*64 bytes", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ints = re.findall(r"int32_t\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert ints == [("n_frames_data", ""), ("n_filled", ""), ("n_flipped", ""), ("iterations", ""), ("status", ""), ("n_soft", ""), ("reserved", "2")]


def test_null_detector_is_refused():
    L = _lib.load()
    b = RC.mixed()
    n, mt = b.obs.shape
    n_seq = len(b.seq_start) - 1
    obs, seed, Kc = np.ascontiguousarray(b.obs), np.ascontiguousarray(b.seed), np.ascontiguousarray(SC.K)
    out = np.full(n * _lib.CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    res = np.full(n_seq * 64, 0xAB, dtype=np.uint8)
    start = np.ascontiguousarray(b.seq_start, dtype=np.int32)
    rc = L.asl_smooth_robust_sequences_batch(None, obs.ctypes.data, n, mt, b.rec.ctypes.data, len(b.rec), Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0,
                                             SC.TAG, seed.ctypes.data, start.ctypes.data_as(C.POINTER(C.c_int32)), n_seq, *b.sigmas, b.huber,
                                             b.max_iters, out.ctypes.data, res.ctypes.data, None)
    assert rc == -1 and b"detector" in L.asl_last_error()
    assert (out == 0xAB).all() and (res == 0xAB).all()


def test_python_surface_has_the_argument():
    import inspect
    from aprilslam_amd.smooth import SmoothResult
    from aprilslam_amd.tag_detector import TagDetector
    for fn in (_lib.Detector.smooth, _lib.Detector.smooth_sequences, TagDetector.localize_sequence, TagDetector.localize_sequences):
        assert inspect.signature(fn).parameters["huber_px"].default == 0.0, fn
    poses = np.zeros(3, dtype=_lib.CAM_POSE_DTYPE)
    poses["n_rejected"] = [0, 2, 1]
    result = np.zeros((), dtype=_lib.SMOOTH_RESULT_DTYPE)
    result["n_soft"] = 3
    r = SmoothResult(poses, result)
    assert r.n_soft == 3 and r.soft.tolist() == [False, True, True]


def test_batches_are_what_the_issue_says():
    b = RC.ragged()
    assert b.seq_start.tolist() == [0, 1, 3, 6, 11, 76] and b.obs.shape == (76, 4) and b.huber == 0.6 and b.max_iters == 3
    m = RC.mixed()
    assert np.diff(m.seq_start).tolist() == [5, 5, 1, 2] and m.obs.shape[1] == 4
    assert m.obs[:5].tobytes() == SC.shape(5, 4, 0)[0].tobytes() and m.obs[5:10].tobytes() != m.obs[:5].tobytes()
    assert [s for s in RC.SHAPES if s[0] == 5] == [(5, 1, 0), (5, 1, 5), (5, 4, 0), (5, 4, 5), (5, 20, 0), (5, 20, 5)] and len(RC.SHAPES) == 18
    obs = RC.shape(65, 20, 0)[0]
    clean = SC.shape(65, 20, 0)[0]
    d = obs["corners"].astype(np.float64) - clean["corners"].astype(np.float64)
    frames = np.flatnonzero(np.abs(d).reshape(65, -1).max(axis=1))
    assert frames.tolist() == list(range(0, 65, 3)) and not d[:, 1:].any() and not d[:, 0, 2:].any()
    assert np.allclose(d[frames, 0, :2], RC.SHAPE_MOVE, atol=1e-3)
    so, _, _, _ = RC.scene()
    co = SC.noise()[0]
    changed = sorted(set(zip(*[x.tolist() for x in np.nonzero(np.abs(so["corners"] - co["corners"]).max(axis=2))])))
    assert changed == sorted([(f, s) for f, s, _, _ in RC.SCENE_MOVED] + [(f, s) for f, s, _ in RC.SCENE_SWAPPED]) and len(changed) == 5
    for f, s, c, dd in RC.SCENE_MOVED:
        assert 8.0 <= np.hypot(*dd) <= 11.0
