"""The ABI of rig tag location: include/aprilslam.h declares asl_locate_tags_rig_frames_device / asl_locate_tags_rig_batch
as the single-camera pair with n_cams after the block and the camera table in place of K, dist, n_dist; the library exports
the two symbols, the ctypes argument lists agree, the entry points refuse a NULL detector before they touch a device or an
output, and the Python surface is there.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from aprilslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("asl_locate_tags_frames_device", "asl_locate_tags_rig_frames_device", "d_"), ("asl_locate_tags_batch", "asl_locate_tags_rig_batch", ""))


def prototype(name):
    """the parameter names of a function declared in the header"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aprilslam.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "%s is not declared" % name
    return [re.sub(r"[\s*]+", " ", p).strip().split(" ")[-1] for p in m.group(1).split(",")]


def test_header_prototypes():
    for one, rig, d in PAIRS:
        a, b = prototype(one), prototype(rig)
        k = a.index("K")
        assert a[k:k + 3] == ["K", "dist", "n_dist"]
        assert b == a[:2] + ["n_cams"] + a[2:k] + [d + "rig"] + a[k + 3:], rig


def test_exports_and_argtypes():
    L = _lib.load()
    for one, rig, _ in PAIRS:
        assert rig in _lib.EXPORTS and hasattr(L, rig)
        a, b = getattr(L, one).argtypes, getattr(L, rig).argtypes
        k = prototype(one).index("K")
        assert b == a[:2] + [C.c_int] + a[2:k] + [C.c_void_p] + a[k + 3:], rig
        assert len(b) == len(prototype(rig))
    assert L.asl_locate_tags_rig_frames_device.argtypes == L.asl_locate_tags_rig_batch.argtypes + [C.c_void_p]


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.zeros((2, 2, 4), dtype=_lib.OBS_DTYPE)
    poses = np.zeros(2, dtype=_lib.CAM_POSE_DTYPE)
    rig = np.zeros(2, dtype=_lib.RIG_CAMERA_DTYPE)
    rig["K"], rig["E"] = np.eye(3), np.eye(4)[:3]
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (3 * 104, 3 * 40, 3 * 304)]
    ptrs = [o.ctypes.data for o in outs]
    assert L.asl_locate_tags_rig_batch(None, obs.ctypes.data, 2, 2, 4, poses.ctypes.data, ptrs[0], 3, rig.ctypes.data, 10.0, 0.0, 2, 0.0, ptrs[1], ptrs[2]) == -1
    assert b"detector" in L.asl_last_error()
    assert L.asl_locate_tags_rig_frames_device(None, None, 2, 2, 4, None, ptrs[0], 3, None, 10.0, 0.0, 2, 0.0, ptrs[1], ptrs[2], None) == -1
    assert b"detector" in L.asl_last_error()
    assert all((o == 0xAB).all() for o in outs)


def test_python_surface():
    from aprilslam_amd import locate
    from aprilslam_amd.rig import Rig
    p = inspect.signature(_lib.Detector.locate_tags_rig).parameters
    assert list(p)[:6] == ["self", "obs", "poses", "tag_map", "rig", "tag_size"]
    assert (p["max_view_rms_px"].default, p["min_views"].default, p["sigma_px"].default) == (0.0, 2, None)
    p = inspect.signature(_lib.Detector.locate_tags_rig_device).parameters
    assert list(p)[:11] == ["self", "obs_ptr", "n_cams", "n_frames", "max_tags", "poses_ptr", "map_ptr", "n_ids", "rig_ptr", "fit_ptr", "tag_size"]
    assert p["cov_ptr"].default is None and p["stream"].default == 0
    # locate_tags_device with n_cams and rig_ptr: the rest of the two lists is the same
    one = [k for k in inspect.signature(_lib.Detector.locate_tags_device).parameters if k not in ("K", "dist")]
    assert [k for k in p if k not in ("n_cams", "rig_ptr")] == one
    assert list(inspect.signature(Rig.locate_tags).parameters)[:6] == ["self", "det", "obs", "poses", "tag_map", "tag_size"]
    p = inspect.signature(Rig.extend_map).parameters
    assert list(p) == ["self", "det", "obs", "tag_map", "tag_size", "tag_sizes", "max_view_rms_px", "min_views", "sigma_px", "max_tag_rms_px"]
    assert (p["tag_sizes"].default, p["max_view_rms_px"].default, p["min_views"].default, p["sigma_px"].default, p["max_tag_rms_px"].default) == \
        (None, 0.0, 2, None, 0.0)
    # the same list as locate.extend_map's, less the one camera's K and dist
    assert [k for k in inspect.signature(locate.extend_map).parameters if k not in ("K", "dist")] == list(p)[1:]


def test_the_record_block_of_extend_map_is_built_once():
    """locate.wanted_records, which locate.extend_map and Rig.extend_map both call: the block grows to every id seen (by any
    camera), the sizes go into the entries without a pose, the entries the map had keep their bytes, the input is not touched"""
    from aprilslam_amd import locate
    from aprilslam_amd.localize import TagMap
    tm = TagMap()
    tm[0] = np.eye(4)
    tm[2] = np.eye(4)
    before = tm.as_records().copy()
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    obs["id"][0, 1, 0], obs["flags"][0, 1, 0] = 1, 3
    obs["id"][1, 2, 3], obs["flags"][1, 2, 3] = 6, 1
    obs["id"][1, 0, 0] = 9                                                    # flags 0: not seen
    rec = locate.wanted_records(obs, tm, {1: 25.0, 2: 30.0, 40: 5.0})
    assert len(rec) == 7 and rec["valid"].tolist() == [1, 0, 1, 0, 0, 0, 0]
    assert rec["size"].tolist() == [0, 25.0, 0, 0, 0, 0, 0]                   # id 2 has a pose: its size is the map's
    assert rec[:3][[0, 2]].tobytes() == before[[0, 2]].tobytes() and tm.as_records().tobytes() == before.tobytes()
    assert len(locate.wanted_records(obs[:, :1], tm)) == 3                    # nothing new seen: a copy of the map's block
    for bad in (-1.0, np.inf, np.nan):
        try:
            locate.wanted_records(obs, tm, {1: bad})
            raise AssertionError("a bad size must fail")
        except ValueError:
            pass
    src = inspect.getsource(locate.extend_map) + inspect.getsource(__import__("aprilslam_amd.rig", fromlist=["Rig"]).Rig.extend_map)
    assert src.count("wanted_records(") == 2 and "np.zeros" not in src
