"""The ABI of rectification into rotated views: include/aprilslam.h declares asl_rectify_views_device /
asl_rectify_views_u8 with the argument names of their documentation, asl_rectify_view with the fields RECTIFY_VIEW_DTYPE
has at the same offsets, and the three constants; the library exports the two symbols, the ctypes argument lists agree,
the entry points refuse a NULL detector before they touch a device or an output, and the Python surface is there.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from aprilslam_amd import _lib
from test_smooth_cov_abi import prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = ["K", "dist", "n_dist", "lens_model", "views", "n_views", "theta_max", "fill"]


def header():
    return open(os.path.join(ROOT, "include", "aprilslam.h")).read()


def test_header_prototypes():
    assert prototype("asl_rectify_views_device") == ["det", "d_src", "n_frames", "channels", "w", "h", "stride", "frame_pitch", "d_dst", "w_out", "h_out",
                                                     "stride_out", "frame_pitch_out"] + LENS + ["stream"]
    assert prototype("asl_rectify_views_u8") == ["det", "src", "channels", "w", "h", "stride", "dst", "w_out", "h_out", "stride_out", "view_pitch_out"] + LENS


def test_the_record_is_144_bytes_with_the_headers_fields_at_the_dtypes_offsets():
    body = re.search(r"typedef struct \{([^}]*)\}\s*asl_rectify_view;", header(), flags=re.S).group(1)
    fields = re.findall(r"double\s+(\w+)\[(\d+)\];", body)
    assert fields == [("K", "9"), ("R", "9")]
    assert [f[0] for f in fields] == list(_lib.RECTIFY_VIEW_DTYPE.names)
    off = 0
    for name, n in fields:
        dt, at = _lib.RECTIFY_VIEW_DTYPE.fields[name][:2]
        assert at == off and dt.shape == (3, 3) and dt.base == np.dtype("<f8"), name
        off += 8 * int(n)
    assert off == 144 == _lib.RECTIFY_VIEW_DTYPE.itemsize


def test_constants():
    got = {k: int(v) for k, v in re.findall(r"#define (ASL_LENS_BROWN|ASL_LENS_FISHEYE|ASL_MAX_VIEWS) (\d+)", header())}
    assert got == {"ASL_LENS_BROWN": 0, "ASL_LENS_FISHEYE": 1, "ASL_MAX_VIEWS": 16}
    assert (_lib.LENS_BROWN, _lib.LENS_FISHEYE, _lib.MAX_VIEWS) == (0, 1, 16)
    assert _lib.LENS_MODELS == {"brown": 0, "fisheye": 1}
    from aprilslam_amd import rig
    assert _lib.MAX_VIEWS == rig.MAX_CAMERAS  # every view is a camera of the rig


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_rectify_views_device", "asl_rectify_views_u8"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(prototype(name)), name
    for name in ("asl_rectify_views_device", "asl_rectify_views_u8"):
        a, names = getattr(L, name).argtypes, prototype(name)
        assert a[names.index("theta_max")] == C.c_double and a[names.index("lens_model")] == C.c_int and a[names.index("n_views")] == C.c_int
        assert a[names.index("views")] == C.c_void_p
    a, names = L.asl_rectify_views_u8.argtypes, prototype("asl_rectify_views_u8")
    assert a[names.index("view_pitch_out")] == C.c_size_t
    # the lens and view arguments follow the frame arguments of the existing pair
    old, new = prototype("asl_rectify_frames_device"), prototype("asl_rectify_views_device")
    assert new[:16] == old[:16] and old[16:] == ["K_new", "fill", "stream"]


def test_null_detector_is_refused():
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    K = np.array([[30.0, 0, 16], [0, 30.0, 8], [0, 0, 1]])
    views = np.zeros(1, dtype=_lib.RECTIFY_VIEW_DTYPE)
    views["K"][0], views["R"][0] = K, np.eye(3)
    src = np.full(32 * 16, 7, dtype=np.uint8)
    dst = np.full(32 * 16, 0xAB, dtype=np.uint8)
    lens = (K.ctypes.data_as(dp), None, 0, 1, views.ctypes.data, 1, 0.0, 0)
    assert L.asl_rectify_views_u8(None, src.ctypes.data, 1, 32, 16, 32, dst.ctypes.data, 32, 16, 32, 32 * 16, *lens) == -1
    assert b"detector" in L.asl_last_error()
    assert L.asl_rectify_views_device(None, src.ctypes.data, 1, 1, 32, 16, 32, 32 * 16, dst.ctypes.data, 32, 16, 32, 32 * 16, *lens, None) == -1
    assert b"detector" in L.asl_last_error()
    assert (dst == 0xAB).all()


def test_python_surface():
    from aprilslam_amd import rectify
    from aprilslam_amd.tag_detector import TagDetector
    p = inspect.signature(_lib.Detector.rectify_views).parameters
    assert list(p)[:5] == ["self", "image", "K", "dist", "views"] and {"model", "size", "theta_max", "fill"} <= set(p)
    p = inspect.signature(_lib.Detector.rectify_views_device).parameters
    assert list(p)[:10] == ["self", "src_ptr", "n_frames", "channels", "width", "height", "dst_ptr", "K", "dist", "views"]
    assert {"model", "theta_max", "fill", "stride", "frame_pitch", "stride_out", "frame_pitch_out", "stream"} <= set(p)
    p = inspect.signature(rectify.distort_points).parameters
    assert list(p) == ["pts", "K", "dist", "K_new", "R", "model", "theta_max"]
    assert (p["K_new"].default, p["R"].default, p["model"].default, p["theta_max"].default) == (None, None, "brown", None)
    assert list(inspect.signature(rectify.undistort_points).parameters) == ["pts", "K", "dist", "K_new", "R", "model"]
    assert list(inspect.signature(rectify.ViewSet.__init__).parameters) == ["self", "K", "dist", "model", "views", "size", "theta_max", "fill"]
    assert list(inspect.signature(rectify.ViewSet.fan).parameters)[:8] == ["K", "dist", "model", "n_views", "hfov_deg", "size", "step_deg", "axis"]
    assert list(inspect.signature(rectify.ViewSet.observe_device).parameters)[:10] == ["self", "det", "src_ptr", "n_frames", "channels", "w", "h",
                                                                                      "tag_size", "max_tags", "stream"]
    for name in ("rig", "rectify", "rectify_device", "save", "load"):
        assert callable(getattr(rectify.ViewSet, name))
    assert inspect.signature(TagDetector.__init__).parameters["lens_model"].default == "brown"


def test_python_refusals_need_no_gpu():
    """what the Python layer refuses before it reaches the library"""
    import pytest

    from aprilslam_amd import rectify
    K = np.array([[190.0, 0, 320], [0, 190.0, 240], [0, 0, 1]])
    with pytest.raises(ValueError):
        rectify.ViewSet(K, [0.1] * 5, "fisheye", [(K, np.eye(3))], (64, 48))      # a fisheye has 0 or 4 coefficients
    with pytest.raises(ValueError):
        rectify.ViewSet(K, None, "pinhole", [(K, np.eye(3))], (64, 48))
    with pytest.raises(ValueError):
        rectify.ViewSet(K, None, "fisheye", [(K, 2 * np.eye(3))], (64, 48))       # not a rotation
    with pytest.raises(ValueError):
        rectify.ViewSet(K, None, "fisheye", [(K, np.diag([1.0, 1.0, -1.0]))], (64, 48))  # a reflection
    with pytest.raises(ValueError):
        rectify.ViewSet(K, None, "fisheye", [(K, np.eye(3))] * 17, (64, 48))
    with pytest.raises(ValueError):
        rectify.ViewSet(K, None, "fisheye", [(K, np.eye(3))], (64, 48), theta_max=4.0)
    with pytest.raises(ValueError):
        _lib._lens(K, [0.1] * 5, "fisheye")
