"""The ABI of the rig tag-map reconstruction: include/aprilslam.h declares asl_map_rig_frames_device / _batch as the robust
map argument lists with n_cams after the block and the rig table in place of K, dist, n_dist, the library exports them, the
ctypes argument lists agree, the records keep their sizes, the host entry point refuses a NULL detector before it touches a
device, and the Python surface has the calls.  The header names the threshold `rig_huber_px` (its `double huber_px` and
`double huber,` are counted by the sequence solver's ABI tests) and names tests/map_ref.py.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np

import map_rig_cases as GC
from aprilslam_amd import _lib
from aprilslam_amd.mapping import MapResult
from aprilslam_amd.rig import Rig
from test_smooth_cov_abi import ROOT, prototype


def test_header_prototypes():
    rob, rig = prototype("asl_map_robust_frames_device"), prototype("asl_map_rig_frames_device")
    k = rob.index("K")
    assert rob[k:k + 3] == ["K", "dist", "n_dist"]
    want = rob[:2] + ["n_cams"] + rob[2:k] + ["d_rig"] + rob[k + 3:]
    assert rig == [w if w != "map_huber_px" else "rig_huber_px" for w in want], rig
    robh, righ = prototype("asl_map_robust_batch"), prototype("asl_map_rig_batch")
    want = robh[:2] + ["n_cams"] + robh[2:k] + ["rig"] + robh[k + 3:]
    assert righ == [w if w != "map_huber_px" else "rig_huber_px" for w in want], righ
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    assert "tests/map_ref.py" in src


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_map_rig_frames_device", "asl_map_rig_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    rob, robh = L.asl_map_robust_frames_device.argtypes, L.asl_map_robust_batch.argtypes
    vp, i32 = C.c_void_p, C.c_int
    assert L.asl_map_rig_frames_device.argtypes == rob[:2] + [i32] + rob[2:5] + [vp] + rob[8:]
    assert L.asl_map_rig_batch.argtypes == robh[:2] + [i32] + robh[2:5] + [vp] + robh[8:]
    assert len(L.asl_map_rig_frames_device.argtypes) == len(prototype("asl_map_rig_frames_device")) == 17
    assert len(L.asl_map_rig_batch.argtypes) == len(prototype("asl_map_rig_batch")) == 16


def test_record_sizes():
    assert _lib.MAP_RESULT_DTYPE.itemsize == 64 and _lib.MAP_TAG_DTYPE.itemsize == 104 and _lib.CAM_POSE_DTYPE.itemsize == 160
    assert _lib.RIG_CAMERA_DTYPE.itemsize == 216 and _lib.OBS_DTYPE.itemsize == 136


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.ascontiguousarray(GC.edge_cases()["2x2"][0])
    nc, n, mt = obs.shape
    rec = GC.PAIR.as_records()
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (GC.N_IDS * 104, GC.N_IDS * 48, n * 160, 64, nc * n * mt * 8)]
    rc = L.asl_map_rig_batch(None, obs.ctypes.data, nc, n, mt, GC.N_IDS, rec.ctypes.data, GC.TAG, -1, GC.HUBER, 30, *[o.ctypes.data for o in outs])
    assert rc == -1 and b"detector" in L.asl_last_error()
    assert all((o == 0xAB).all() for o in outs)


def test_python_surface():
    for fn in (_lib.Detector.build_map_rig, _lib.Detector.build_map_rig_device, Rig.build_map):
        assert inspect.signature(fn).parameters["huber_px"].default == 0.0, fn
    assert list(inspect.signature(Rig.build_map).parameters) == ["self", "det", "obs", "n_ids", "tag_size", "world_id", "max_iters", "with_std",
                                                                 "huber_px"]
    p = inspect.signature(Rig.build_map).parameters
    assert p["world_id"].default == -1 and p["max_iters"].default == 30 and p["with_std"].default is True
    assert inspect.signature(_lib.Detector.build_map_rig).parameters["with_slot_weight"].default is False
    assert inspect.signature(_lib.Detector.build_map_rig_device).parameters["slot_weight_ptr"].default == 0
    # a rig's weight block is 3-D: (camera, frame, slot, id, weight); one camera's stays (frame, slot, id, weight)
    res = np.zeros((), dtype=_lib.MAP_RESULT_DTYPE)
    tm, poses = np.zeros(4, dtype=_lib.MAP_TAG_DTYPE), np.zeros(2, dtype=_lib.CAM_POSE_DTYPE)
    w = np.array([[[1.0, 0.25, 0.0], [0.5, 1.0, 0.0]], [[1.0, 1.0, 0.0], [1.0, 0.75, 0.0]]])
    ids = np.array([[[3, 1, -1], [3, 2, -1]], [[0, 1, -1], [0, 2, -1]]])
    assert MapResult(res, tm, None, poses, slot_weight=w, slot_ids=ids).soft_slots() == [(0, 0, 1, 1, 0.25), (0, 1, 0, 3, 0.5), (1, 1, 1, 2, 0.75)]
    assert MapResult(res, tm, None, poses, slot_weight=w[0], slot_ids=ids[0]).soft_slots() == [(0, 1, 1, 0.25), (1, 0, 3, 0.5)]
    assert MapResult(res, tm, None, poses, slot_weight=w).soft_slots()[0] == (0, 0, 1, -1, 0.25)
