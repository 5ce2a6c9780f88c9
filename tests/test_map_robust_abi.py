"""The ABI of the robust tag-map reconstruction: include/aprilslam.h declares asl_map_robust_frames_device / _batch as the
plain argument lists with the threshold after world_id and the slot weights after the result, the library exports them, the
ctypes argument lists agree, asl_map_result carries n_soft where its reserved int was, the host entry point refuses a NULL
detector before it touches a device, and the Python surface has the arguments.  The header names the threshold
`map_huber_px`: its `double huber_px` and `double huber` are counted by the sequence solver's ABI tests.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import localize_cases as LC
import map_cases as MC
import map_robust_cases as RC
from aprilslam_amd import _lib
from test_smooth_cov_abi import ROOT, prototype


def test_header_prototypes():
    dev, rob = prototype("asl_map_frames_device"), prototype("asl_map_robust_frames_device")
    at = dev.index("world_id") + 1
    assert rob == dev[:at] + ["map_huber_px"] + dev[at:-1] + ["d_slot_weight", "stream"] and rob[at + 1] == "max_iters"
    host, robh = prototype("asl_map_batch"), prototype("asl_map_robust_batch")
    assert robh == host[:at] + ["map_huber_px"] + host[at:] + ["slot_weight"]


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_map_robust_frames_device", "asl_map_robust_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    dev, host = L.asl_map_frames_device.argtypes, L.asl_map_batch.argtypes
    assert dev[9:11] == [C.c_int, C.c_int]
    assert L.asl_map_robust_frames_device.argtypes == dev[:10] + [C.c_double] + dev[10:-1] + [C.c_void_p, C.c_void_p]
    assert L.asl_map_robust_batch.argtypes == host[:10] + [C.c_double] + host[10:] + [C.c_void_p]
    assert len(L.asl_map_robust_frames_device.argtypes) == len(prototype("asl_map_robust_frames_device")) == 18
    assert len(L.asl_map_robust_batch.argtypes) == len(prototype("asl_map_robust_batch")) == 17


def test_record_layout():
    dt = _lib.MAP_RESULT_DTYPE
    assert dt.itemsize == 64 and dt.names[-2:] == ("status", "n_soft") and "reserved" not in dt.names
    assert dt.fields["n_soft"][1] == 60 and dt.fields["n_soft"][0] == np.dtype("<i4") and dt.fields["status"][1] == 56
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*)\}\s*asl_map_result;\s*/\*\s*64 bytes", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ints = [n.strip() for decl in re.findall(r"int32_t\s+([^;]+);", body) for n in decl.split(",")]
    assert ints == ["n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft"]
    doubles = [n.strip() for decl in re.findall(r"double\s+([^;]+);", body) for n in decl.split(",")]
    assert doubles == ["cost_seed", "cost", "rms_px", "rms_seed_px"]    # 32 bytes, then the eight ints: n_soft at 60


def test_null_detector_is_refused():
    L = _lib.load()
    obs = np.ascontiguousarray(RC.repair_cases()["small_slip"][0])
    n, mt = obs.shape
    Kc = np.ascontiguousarray(RC.K)
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (MC.N_IDS * 104, MC.N_IDS * 48, n * 160, 64, n * mt * 8)]
    rc = L.asl_map_robust_batch(None, obs.ctypes.data, n, mt, MC.N_IDS, Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, LC.TAG_INNER, -1,
                                RC.HUBER, 30, *[o.ctypes.data for o in outs])
    assert rc == -1 and b"detector" in L.asl_last_error()
    assert all((o == 0xAB).all() for o in outs)


def test_python_surface_has_the_arguments():
    from aprilslam_amd.mapping import MapResult
    from aprilslam_amd.tag_detector import TagDetector
    for fn in (_lib.Detector.build_map, _lib.Detector.build_map_device, TagDetector.build_map):
        assert inspect.signature(fn).parameters["huber_px"].default == 0.0, fn
    assert inspect.signature(_lib.Detector.build_map).parameters["with_slot_weight"].default is False
    assert inspect.signature(_lib.Detector.build_map_device).parameters["slot_weight_ptr"].default == 0
    res = np.zeros((), dtype=_lib.MAP_RESULT_DTYPE)
    res["n_soft"] = 2
    tm, poses = np.zeros(4, dtype=_lib.MAP_TAG_DTYPE), np.zeros(2, dtype=_lib.CAM_POSE_DTYPE)
    plain = MapResult(res, tm, None, poses)
    assert plain.n_soft == 2 and plain.slot_weight is None
    try:
        plain.soft_slots()
        raise AssertionError("soft_slots() without weights must fail")
    except ValueError:
        pass
    w = np.array([[1.0, 0.25, 0.0], [0.5, 1.0, 0.0]])
    ids = np.array([[3, 1, -1], [3, 2, -1]])
    assert MapResult(res, tm, None, poses, slot_weight=w, slot_ids=ids).soft_slots() == [(0, 1, 1, 0.25), (1, 0, 3, 0.5)]
