"""The ABI of tag location: include/aprilslam.h declares asl_locate_tags_frames_device / asl_locate_tags_batch with the
argument names of their documentation and asl_tag_fit with the fields TAG_FIT_DTYPE has, at the same offsets; the library
exports the two symbols, the ctypes argument lists agree, the entry points refuse a NULL detector before they touch a
device or an output, and the Python surface is there.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from aprilslam_amd import _lib
from test_smooth_cov_abi import prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["det", "d_obs", "n_frames", "max_tags", "d_poses", "d_map", "n_ids", "K", "dist", "n_dist", "tag_size", "max_view_rms_px", "min_views", "sigma_px"]
C_SIZES = {"double": 8, "int32_t": 4}


def test_header_prototypes():
    assert prototype("asl_locate_tags_frames_device") == HEAD + ["d_fit", "d_cov", "stream"]
    assert prototype("asl_locate_tags_batch") == [p[2:] if p.startswith("d_") else p for p in HEAD] + ["fit", "cov"]


def test_the_record_is_40_bytes_with_the_headers_fields_at_the_dtypes_offsets():
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*asl_tag_fit;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, fields = 0, []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        for name in names.split(","):
            fields.append((name.strip(), off, C_SIZES[ctype]))
            off += C_SIZES[ctype]
    assert off == 40 == _lib.TAG_FIT_DTYPE.itemsize
    assert [f[0] for f in fields] == list(_lib.TAG_FIT_DTYPE.names)
    for name, o, size in fields:
        dt, at = _lib.TAG_FIT_DTYPE.fields[name][:2]
        assert (at, dt.itemsize) == (o, size) and dt.kind == ("f" if size == 8 else "i"), name


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_locate_tags_frames_device", "asl_locate_tags_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(prototype(name)), name
    a = L.asl_locate_tags_batch.argtypes
    assert L.asl_locate_tags_frames_device.argtypes == a + [C.c_void_p]
    names = prototype("asl_locate_tags_batch")
    assert a[names.index("min_views")] == C.c_int and a[names.index("max_view_rms_px")] == C.c_double and a[names.index("sigma_px")] == C.c_double


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.zeros((2, 4), dtype=_lib.OBS_DTYPE)
    poses = np.zeros(2, dtype=_lib.CAM_POSE_DTYPE)
    Kc = np.eye(3)
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (3 * 104, 3 * 40, 3 * 304)]
    ptrs = [o.ctypes.data for o in outs]
    cam = (Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, 10.0)
    assert L.asl_locate_tags_batch(None, obs.ctypes.data, 2, 4, poses.ctypes.data, ptrs[0], 3, *cam, 0.0, 2, 0.0, ptrs[1], ptrs[2]) == -1
    assert b"detector" in L.asl_last_error()
    assert L.asl_locate_tags_frames_device(None, None, 2, 4, None, ptrs[0], 3, *cam, 0.0, 2, 0.0, ptrs[1], ptrs[2], None) == -1
    assert b"detector" in L.asl_last_error()
    assert all((o == 0xAB).all() for o in outs)


def test_python_surface():
    from aprilslam_amd import locate
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.tag_detector import TagDetector
    p = inspect.signature(_lib.Detector.locate_tags).parameters
    assert list(p)[:7] == ["self", "obs", "poses", "map_records", "K", "dist", "tag_size"]
    assert (p["max_view_rms_px"].default, p["min_views"].default, p["sigma_px"].default) == (0.0, 2, None)
    assert "cov_ptr" in inspect.signature(_lib.Detector.locate_tags_device).parameters
    assert list(inspect.signature(locate.extend_map).parameters)[:7] == ["det", "obs", "tag_map", "K", "dist", "tag_size", "tag_sizes"]
    assert list(inspect.signature(TagDetector.extend_map).parameters)[:3] == ["self", "frames_or_obs", "tag_map"]
    assert callable(SLAM.extend_map)
    assert locate.TAG_FIT_DTYPE is _lib.TAG_FIT_DTYPE


def test_the_result_object():
    """LocateResult reads the records: the extended TagMap keeps the sizes, located_ids and tag_std follow the statuses"""
    from aprilslam_amd.locate import LocateResult
    rec = np.zeros(4, dtype=_lib.MAP_TAG_DTYPE)
    rec["T"][:, [0, 5, 10]] = 1.0
    rec["valid"][[0, 2, 3]] = 1
    rec["size"][2] = 20.0
    fit = np.zeros(4, dtype=_lib.TAG_FIT_DTYPE)
    fit["status"] = [1, 2, 0, 0]
    cov = np.zeros(4, dtype=_lib.POSE_COV_DTYPE)
    cov["status"] = [1, 1, 0, 2]
    cov["cov"][2] = np.diag([1e-6, 4e-6, 9e-6, 0.01, 0.04, 0.09])
    r = LocateResult(rec, fit, cov)
    assert r.located_ids == [2, 3] and r.status.tolist() == [1, 2, 0, 0]
    assert r.tag_map.ids() == [0, 2, 3] and r.tag_map.size(2) == 20.0
    std = r.tag_std()
    assert list(std) == [2] and np.allclose(std[2][0], [1e-3, 2e-3, 3e-3]) and np.allclose(std[2][1], [0.1, 0.2, 0.3])
    try:
        LocateResult(rec, fit).tag_std()
        raise AssertionError("tag_std without a covariance must fail")
    except ValueError:
        pass
