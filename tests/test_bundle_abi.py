"""The ABI of the tag-bundle calls: include/aprilslam.h declares the six entry points, the library exports them, the ctypes
argument lists agree with the prototypes, asl_bundle_rel has the size and field offsets of BUNDLE_REL_DTYPE, a NULL detector
is refused before a device or an output is touched, and the Python surface is there.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from aprilslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asl_localize_bundles_frames_device", "asl_localize_bundles_batch", "asl_localize_bundles_rig_frames_device",
         "asl_localize_bundles_rig_batch", "asl_bundle_relative_device", "asl_bundle_relative_batch")


def header():
    return open(os.path.join(ROOT, "include", "aprilslam.h")).read()


def prototype(name):
    """the parameter names of a function declared in the header"""
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "%s is not declared" % name
    return [re.sub(r"[\s*]+", " ", p).strip().split(" ")[-1] for p in m.group(1).split(",")]


def test_the_six_exports_resolve():
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == len(prototype(name)), name


def test_prototypes_follow_the_one_map_calls():
    """the bundle forms are the one-map covariance forms with n_bundles after the tables; the device forms end in the stream"""
    for bundle, one, d in (("asl_localize_bundles_frames_device", "asl_localize_cov_frames_device", "d_"), ("asl_localize_bundles_batch", "asl_localize_cov_batch", ""),
                           ("asl_localize_bundles_rig_frames_device", "asl_localize_rig_cov_frames_device", "d_"),
                           ("asl_localize_bundles_rig_batch", "asl_localize_rig_cov_batch", "")):
        a, b = prototype(one), prototype(bundle)
        k = a.index(d + "map")
        assert b == a[:k] + [d + "maps", "n_bundles"] + a[k + 1:], bundle
        L = _lib.load()
        ta, tb = getattr(L, one).argtypes, getattr(L, bundle).argtypes
        assert tb == ta[:k + 1] + [C.c_int] + ta[k + 1:], bundle
    assert prototype("asl_bundle_relative_device") == ["det", "d_poses", "d_cov", "n_frames", "n_bundles", "ref", "d_rel", "stream"]
    assert prototype("asl_bundle_relative_batch") == ["det", "poses", "cov", "n_frames", "n_bundles", "ref", "rel"]


def test_record_layout():
    """asl_bundle_rel in the header: the fields of BUNDLE_REL_DTYPE in order, at its offsets, 424 bytes"""
    m = re.search(r"typedef struct \{([^}]*)\}\s*asl_bundle_rel;\s*/\*\s*(\d+) bytes", header(), flags=re.S)
    assert m, "asl_bundle_rel is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(double|int32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    size = {"double": 8, "int32_t": 4}
    off, want = 0, []
    for ty, name, n in fields:
        want.append((name, off))
        off += size[ty] * int(n or 1)
    dt = _lib.BUNDLE_REL_DTYPE
    assert [(n, dt.fields[n][1]) for n in dt.names] == want == [("T", 0), ("cov", 128), ("status", 416), ("reserved", 420)]
    assert off == dt.itemsize == int(m.group(2)) == 424
    assert dt["T"].shape == (4, 4) and dt["cov"].shape == (6, 6)
    from aprilslam_amd import bundles, localize
    assert localize.BUNDLE_REL_DTYPE is dt and bundles.BUNDLE_REL_DTYPE is dt and "BUNDLE_REL_DTYPE" in localize.__all__


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.zeros((2, 2, 4), dtype=_lib.OBS_DTYPE)
    maps = np.zeros((3, 5), dtype=_lib.MAP_TAG_DTYPE)
    rig = np.zeros(2, dtype=_lib.RIG_CAMERA_DTYPE)
    rig["K"], rig["E"] = np.eye(3), np.eye(4)[:3]
    K = np.eye(3)
    Kp = K.ctypes.data_as(C.POINTER(C.c_double))
    out, cov, rel = (np.full(6 * n, 0xAB, dtype=np.uint8) for n in (160, 304, 424))
    poses = np.zeros((2, 3), dtype=_lib.CAM_POSE_DTYPE)
    calls = [lambda: L.asl_localize_bundles_batch(None, obs.ctypes.data, 2, 4, maps.ctypes.data, 3, 5, Kp, None, 0, 10.0, 0.0, 0.0, out.ctypes.data, cov.ctypes.data),
             lambda: L.asl_localize_bundles_frames_device(None, None, 2, 4, None, 3, 5, Kp, None, 0, 10.0, 0.0, 0.0, out.ctypes.data, cov.ctypes.data, None),
             lambda: L.asl_localize_bundles_rig_batch(None, obs.ctypes.data, 2, 2, 4, maps.ctypes.data, 3, 5, rig.ctypes.data, 10.0, 0.0, 0.0, out.ctypes.data,
                                                      cov.ctypes.data),
             lambda: L.asl_localize_bundles_rig_frames_device(None, None, 2, 2, 4, None, 3, 5, None, 10.0, 0.0, 0.0, out.ctypes.data, cov.ctypes.data, None),
             lambda: L.asl_bundle_relative_batch(None, poses.ctypes.data, None, 2, 3, 0, rel.ctypes.data),
             lambda: L.asl_bundle_relative_device(None, None, None, 2, 3, 0, rel.ctypes.data, None)]
    for call in calls:
        assert call() == -1
        assert b"detector" in L.asl_last_error() or b"NULL" in L.asl_last_error()
    assert (out == 0xAB).all() and (cov == 0xAB).all() and (rel == 0xAB).all()


def test_python_surface():
    from aprilslam_amd.bundles import BundleResult, BundleSet
    from aprilslam_amd.rig import Rig
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.tag_detector import TagDetector
    D = _lib.Detector
    # the bundle methods follow localize / localize_rig: the map argument becomes the bundles, map_cov goes
    for one, bundle in (("localize", "localize_bundles"), ("localize_rig", "localize_bundles_rig")):
        a, b = list(inspect.signature(getattr(D, one)).parameters), list(inspect.signature(getattr(D, bundle)).parameters)
        assert b == [("bundles" if k == "tag_map" else k) for k in a if k != "map_cov"], bundle
    for one, bundle in (("localize_device", "localize_bundles_device"), ("localize_rig_device", "localize_bundles_rig_device")):
        a, b = list(inspect.signature(getattr(D, one)).parameters), list(inspect.signature(getattr(D, bundle)).parameters)
        want = []
        for k in a:
            if k != "map_cov":
                want += ["maps_ptr", "n_bundles"] if k == "map_ptr" else [k]
        assert b == want, bundle
    assert list(inspect.signature(D.bundle_relative).parameters) == ["self", "poses", "cov", "ref"]
    assert list(inspect.signature(D.bundle_relative_device).parameters) == ["self", "poses_ptr", "cov_ptr", "n_frames", "n_bundles", "ref", "rel_ptr", "stream"]
    p = inspect.signature(TagDetector.localize_bundles).parameters
    assert list(p) == ["self", "dets", "poses", "n_per_frame", "bundles", "ref", "max_tag_rms_px", "with_cov", "sigma_px", "max_tags"]
    assert [p[k].default for k in list(p)[5:]] == [None, 0.0, False, 0.0, None]
    assert list(inspect.signature(SLAM.localize_bundles).parameters)[:5] == ["self", "dets", "poses", "n_per_frame", "bundles"]
    p = inspect.signature(Rig.localize_bundles).parameters
    assert list(p) == ["self", "det", "obs", "bundles", "tag_size", "max_tag_rms_px", "with_cov", "sigma_px"]
    for name in ("table", "save", "load", "from_map"):
        assert hasattr(BundleSet, name)
    for name in ("T", "status", "cov", "relative", "pose_std"):
        assert hasattr(BundleResult, name)
