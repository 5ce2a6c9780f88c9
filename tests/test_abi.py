"""The C-ABI library loads and exports every symbol include/aprilslam.h declares; without a GPU the
product path fails loudly instead of falling back to anything."""
import os
import re

import numpy as np
import pytest

from aprilslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asl_[a-z0-9_]+)\s*\(", src)))


def test_header_functions_are_exported():
    L = _lib.load()
    names = declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), "libaprilslam.so does not export %s" % n
    assert set(_lib.EXPORTS) == set(names)
    assert b"gfx950" in L.asl_version()


def test_record_dtypes_have_the_header_layout():
    """The ABI's records as numpy dtypes: the header's sizes, and every field where a C compiler puts it (the same fields
    laid out with C alignment land at the same offsets)."""
    assert _lib.DET_DTYPE.itemsize == 4 + 4 + 4 + 4 + 16 + 64
    assert _lib.POSE_DTYPE.itemsize == 24 + 24 + 128 + 8
    for name in ("DET_DTYPE", "POSE_DTYPE", "QUAD_DTYPE", "OBS_DTYPE", "PLANE_DTYPE", "MAP_TAG_DTYPE", "CAM_POSE_DTYPE",
                 "CALIB_RESULT_DTYPE", "MAP_RESULT_DTYPE"):
        dt = getattr(_lib, name)
        c = np.dtype(dt.descr, align=True)
        assert c.itemsize == dt.itemsize and [c.fields[f][1] for f in c.names] == [dt.fields[f][1] for f in dt.names], name


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.AslError):
        _lib.Detector("tagStandard41h12")
    from aprilslam_amd.apriltag import apriltag
    with pytest.raises(RuntimeError):
        apriltag("tagStandard41h12")


def test_product_does_not_touch_the_oracle():
    """Nothing under aprilslam_amd/ (or the drop-in shim) may import, link or open oracle/."""
    bad = []
    for base in ("aprilslam_amd", "lib"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".inc", ".h", ".cpp")):
                    txt = open(os.path.join(dp, f), errors="replace").read()
                    if re.search(r"oracle_lib|liboracle|oracle/|aso_", txt):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_reference_shim_location():
    """`from apriltag import apriltag` resolves from the directory the reference puts on sys.path
    (reference src/detection/tag_detector.py:7-9)."""
    import importlib.util
    p = os.path.join(ROOT, "lib", "apriltag", "build", "apriltag.py")
    spec = importlib.util.spec_from_file_location("apriltag_shim_test", p)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    from aprilslam_amd.apriltag import apriltag as impl
    assert m.apriltag is impl
