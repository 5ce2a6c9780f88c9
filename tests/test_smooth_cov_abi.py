"""The ABI of the smoothed poses' covariance: include/aprilslam.h declares the two entry points next to the plain ones, the
library exports them, the ctypes argument lists are the plain calls' plus the covariance pointer, and the record is the
304-byte asl_pose_cov.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

from aprilslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prototype(name):
    """the parameter names of a function declared in the header"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aprilslam.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
    assert m, "%s is not declared" % name
    return [re.sub(r"[\s*]+", " ", p).strip().split(" ")[-1] for p in m.group(1).split(",")]


def test_header_prototypes():
    plain, cov = prototype("asl_smooth_frames_device"), prototype("asl_smooth_cov_frames_device")
    assert cov == plain[:-1] + ["d_cov", "stream"]
    plain, cov = prototype("asl_smooth_batch"), prototype("asl_smooth_cov_batch")
    assert cov == plain + ["cov"]


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_smooth_cov_frames_device", "asl_smooth_cov_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    vp = C.c_void_p
    assert L.asl_smooth_cov_frames_device.argtypes == L.asl_smooth_frames_device.argtypes[:-1] + [vp, vp]
    assert L.asl_smooth_cov_batch.argtypes == L.asl_smooth_batch.argtypes + [vp]
    assert len(L.asl_smooth_cov_frames_device.argtypes) == len(prototype("asl_smooth_cov_frames_device")) == 19
    assert len(L.asl_smooth_cov_batch.argtypes) == len(prototype("asl_smooth_cov_batch")) == 18


def test_record_layout():
    dt = _lib.POSE_COV_DTYPE
    assert dt.itemsize == 304 and dt.names == ("cov", "sigma_px", "dof", "status")
    assert [dt.fields[f][1] for f in dt.names] == [0, 288, 296, 300]
    c = np.dtype(dt.descr, align=True)
    assert c.itemsize == dt.itemsize and [c.fields[f][1] for f in c.names] == [dt.fields[f][1] for f in dt.names]
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    assert re.search(r"\}\s*asl_pose_cov;\s*/\*\s*304 bytes", src)
