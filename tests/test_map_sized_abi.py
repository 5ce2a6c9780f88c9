"""The ABI of the sized tag-map reconstruction: include/aprilslam.h declares asl_map_sized_* and asl_map_rig_sized_* as the
robust and the rig argument lists with `tag_sizes` directly after tag_size, the library exports them, the ctypes argument
lists agree, the host entry points refuse a NULL detector before they touch a device or an output, and the Python surface
has tag_sizes.  The header names the threshold `sized_huber_px`: `double huber_px` is counted by the sequence solver's ABI
tests.  No GPU."""
import ctypes as C
import inspect

import numpy as np

import map_sized_cases as ZC
from aprilslam_amd import _lib
from test_smooth_cov_abi import prototype

PAIRS = (("asl_map_robust_frames_device", "asl_map_sized_frames_device", "map_huber_px"), ("asl_map_robust_batch", "asl_map_sized_batch", "map_huber_px"),
         ("asl_map_rig_frames_device", "asl_map_rig_sized_frames_device", "rig_huber_px"), ("asl_map_rig_batch", "asl_map_rig_sized_batch", "rig_huber_px"))


def test_header_prototypes():
    for old, new, huber in PAIRS:
        a, b = prototype(old), prototype(new)
        at = a.index("tag_size") + 1
        assert b == a[:at] + ["tag_sizes"] + [("sized_huber_px" if p == huber else p) for p in a[at:]], new


def test_exports_and_argtypes():
    L = _lib.load()
    for old, new, _ in PAIRS:
        assert new in _lib.EXPORTS and hasattr(L, new)
        a, b = getattr(L, old).argtypes, getattr(L, new).argtypes
        at = prototype(old).index("tag_size") + 1
        assert a[at - 1] == C.c_double and b == a[:at] + [C.POINTER(C.c_float)] + a[at:], new
        assert len(b) == len(prototype(new))


def test_null_detector_is_refused():
    L = _lib.load()
    obs, rig, t = ZC.edge_cases()["behind"]
    obs = np.ascontiguousarray(obs)
    nc, n, mt = obs.shape
    rec = rig.as_records()
    Kc = np.ascontiguousarray(rig.cameras[0].K)
    tp = t.ctypes.data_as(C.POINTER(C.c_float))
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (ZC.N_IDS * 104, ZC.N_IDS * 48, n * 160, 64, nc * n * mt * 8)]
    ptrs = [o.ctypes.data for o in outs]
    rc = L.asl_map_sized_batch(None, obs[0].ctypes.data, n, mt, ZC.N_IDS, Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, ZC.TAG, tp, -1, ZC.HUBER,
                               30, *ptrs)
    assert rc == -1 and b"detector" in L.asl_last_error()
    rc = L.asl_map_rig_sized_batch(None, obs.ctypes.data, nc, n, mt, ZC.N_IDS, rec.ctypes.data, ZC.TAG, tp, -1, ZC.HUBER, 30, *ptrs)
    assert rc == -1 and b"detector" in L.asl_last_error()
    for fn, head in ((L.asl_map_sized_frames_device, (None, None, n, mt, ZC.N_IDS, Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, ZC.TAG, tp)),
                     (L.asl_map_rig_sized_frames_device, (None, None, nc, n, mt, ZC.N_IDS, None, ZC.TAG, tp))):
        assert fn(*head, -1, ZC.HUBER, 30, *ptrs, None) == -1 and b"detector" in L.asl_last_error()
    assert all((o == 0xAB).all() for o in outs)


def test_python_surface_has_the_argument():
    from aprilslam_amd.rig import Rig
    from aprilslam_amd.tag_detector import TagDetector
    for fn in (_lib.Detector.build_map, _lib.Detector.build_map_device, _lib.Detector.build_map_rig, _lib.Detector.build_map_rig_device,
               TagDetector.build_map):
        assert inspect.signature(fn).parameters["tag_sizes"].default is None, fn
    # Rig.build_map's parameter list is pinned (tests/test_map_rig_abi.py): the rig's sized form is a method of its own
    assert list(inspect.signature(Rig.build_map_sized).parameters)[:6] == ["self", "det", "obs", "n_ids", "tag_size", "tag_sizes"]


def test_the_size_table_helper():
    t = _lib._size_table({3: 20.0, 70: 5.0, 0: 2.5}, 8)
    assert t.dtype == np.float32 and t.tolist() == [2.5, 0, 0, 20.0, 0, 0, 0, 0]           # ids >= n_ids are ignored
    assert _lib._size_table(np.arange(8.0), 8).tolist() == list(range(8))
    for bad in (np.zeros(7), np.zeros(9)):
        try:
            _lib._size_table(bad, 8)
            raise AssertionError("a table of the wrong length must fail")
        except ValueError:
            pass


def test_a_map_with_sizes_round_trips_through_the_result(tmp_path):
    """MapResult.tag_map carries the size field, through save() and load()"""
    from aprilslam_amd.localize import TagMap
    from aprilslam_amd.mapping import MapResult
    rec = np.zeros(4, dtype=_lib.MAP_TAG_DTYPE)
    rec["T"][:, [0, 5, 10]] = 1.0
    rec["valid"][[0, 2]] = 1
    rec["size"][2] = 20.0
    tm = MapResult(np.zeros((), dtype=_lib.MAP_RESULT_DTYPE), rec, None, np.zeros(1, dtype=_lib.CAM_POSE_DTYPE)).tag_map
    assert tm.ids() == [0, 2] and tm.size(2) == 20.0 and tm.size(0) == 0.0
    path = str(tmp_path / "map.npz")
    tm.save(path)
    back = TagMap.load(path).as_records()
    assert back["size"].tolist() == [0.0, 0.0, 20.0] and back["valid"].tolist() == [1, 0, 1]
