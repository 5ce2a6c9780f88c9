"""The covariance forms on the call paths of aprilslam_amd._lib, on a Detector that owns no device (the entry points are
stubbed, as in tests/test_map_call_abi.py): with_cov / cov= choose asl_mapcov_* and asl_mapcov_rig_*, map_cov= chooses
asl_localize_mapcov_* and asl_localize_rig_mapcov_*, each with the number of arguments its header declaration has and the
covariance's three where the declaration has them; the header's argument lists are the sized / _cov ones plus those three;
and mapping.MapCovariance.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from aprilslam_amd import _lib
from aprilslam_amd.mapping import MapCovariance, MapResult
from aprilslam_amd.rig import Rig, RigCamera
from test_smooth_cov_abi import prototype

MAP_ENTRIES = [base + form for base in ("asl_mapcov", "asl_mapcov_rig") for form in ("_batch", "_frames_device")]
LOC_ENTRIES = [base + form for base in ("asl_localize_mapcov", "asl_localize_rig_mapcov") for form in ("_batch", "_frames_device")]
K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
N_IDS = 8


class Stub:
    def __init__(self):
        self.calls = []
        for name in MAP_ENTRIES + LOC_ENTRIES:
            setattr(self, name, lambda *a, _n=name: self.calls.append((_n, a)) or 0)


def detector():
    det = object.__new__(_lib.Detector)
    det._L, det._h = Stub(), C.c_void_p(1)
    return det


def value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def last_call(det, entry):
    (name, args), = det._L.calls
    det._L.calls.clear()
    names = prototype(name)
    assert name == entry and len(args) == len(names), (name, len(args), len(names))
    return names, args


def test_header_prototypes():
    for rig in ("", "_rig"):
        sized, cov = prototype("asl_map%s_sized_frames_device" % rig), prototype("asl_mapcov%s_frames_device" % rig)
        hub = [n for n in sized if n.endswith("huber_px")][0]
        assert [n for n in cov if not n.endswith("huber_px")] == [n for n in sized[:-1] if n != hub] + ["d_cov_slot", "d_map_cov", "cap_tags", "stream"]
        sized, cov = prototype("asl_map%s_sized_batch" % rig), prototype("asl_mapcov%s_batch" % rig)
        assert [n for n in cov if not n.endswith("huber_px")] == [n for n in sized if n != hub] + ["cov_slot", "map_cov", "cap_tags"]
        plain, mc = prototype("asl_localize%s_cov_frames_device" % rig), prototype("asl_localize%s_mapcov_frames_device" % rig)
        assert mc == plain[:-1] + ["d_map_cov", "ld", "d_cov_slot", "stream"]
        plain, mc = prototype("asl_localize%s_cov_batch" % rig), prototype("asl_localize%s_mapcov_batch" % rig)
        assert mc == plain + ["map_cov", "ld", "cov_slot"]
    assert set(MAP_ENTRIES + LOC_ENTRIES) <= set(_lib.EXPORTS)


@pytest.mark.parametrize("sized", [False, True])
def test_map_cov_entries(sized):
    det = detector()
    sizes = {3: 2.5} if sized else None
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    obs["id"][:, :, 0], obs["id"][:, :, 1], obs["id"][0, 0, 2], obs["flags"] = 1, 5, 6, 1      # ids 1, 5 and 6 take part: cap_tags 2
    rig = Rig([RigCamera(K), RigCamera(K)])
    for entry, call in (("asl_mapcov_batch", lambda **kw: det.build_map(obs[0], N_IDS, K, None, 0.1, **kw)),
                        ("asl_mapcov_rig_batch", lambda **kw: det.build_map_rig(obs, N_IDS, rig, 0.1, **kw))):
        out = call(world_id=3, max_iters=17, huber_px=1.5, tag_sizes=sizes, with_cov=True)
        assert len(out) == 5 and out[4][0].shape == (N_IDS,) and (out[4][0] == -1).all() and out[4][1].shape == (0, 0)
        names, args = last_call(det, entry)
        t = args[names.index("tag_sizes")]
        assert (t is None) if not sized else [t[i] for i in range(N_IDS)] == [0, 0, 0, 2.5, 0, 0, 0, 0]
        assert args[names.index("cov_huber_px")] == 1.5 and args[names.index("max_iters")] == 17 and args[names.index("world_id")] == 3
        assert args[names.index("cap_tags")] == 2 and args[names.index("cov_slot")] and args[names.index("map_cov")]
        assert args[names.index("slot_weight")] is None
        out = call(with_slot_weight=True, with_cov=True)
        assert len(out) == 6
        names, args = last_call(det, entry)
        assert args[names.index("slot_weight")] and args[names.index("cap_tags")] == 2
    cov = (0x8000, 0x9000, 7)
    det.build_map_device(0x1000, 3, 4, N_IDS, K, None, 0.1, 0x2000, 0, 0x4000, 0x5000, world_id=3, max_iters=17, stream=99, tag_sizes=sizes, cov=cov)
    names, args = last_call(det, "asl_mapcov_frames_device")
    assert [value(args[names.index(n)]) for n in ("d_cov_slot", "d_map_cov", "cap_tags", "stream")] == [0x8000, 0x9000, 7, 99]
    assert value(args[names.index("d_tag_std")]) is None and value(args[names.index("d_slot_weight")]) is None
    det.build_map_rig_device(0x1000, 2, 3, 4, N_IDS, 0x6000, 0.1, 0x2000, 0x3000, 0x4000, 0x5000, stream=99, slot_weight_ptr=0x7000, tag_sizes=sizes, cov=cov)
    names, args = last_call(det, "asl_mapcov_rig_frames_device")
    assert [value(args[names.index(n)]) for n in ("d_slot_weight", "d_cov_slot", "d_map_cov", "cap_tags", "stream")] == [0x7000, 0x8000, 0x9000, 7, 99]


def test_localize_mapcov_entries():
    det = detector()
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    tmap = np.zeros(N_IDS, dtype=_lib.MAP_TAG_DTYPE)
    rig = Rig([RigCamera(K), RigCamera(K)])
    cov = MapCovariance([2, 5], np.eye(12))
    for mc in (cov, (cov.cov_slot(N_IDS), cov.matrix)):
        det.localize(obs[0], tmap, K, None, 0.1, sigma_px=0.0, map_cov=mc)
        names, args = last_call(det, "asl_localize_mapcov_batch")
        assert args[names.index("ld")] == 12 and args[names.index("map_cov")] and args[names.index("cov_slot")]
        det.localize_rig(obs, tmap, rig, 0.1, sigma_px=0.3, map_cov=mc)
        names, args = last_call(det, "asl_localize_rig_mapcov_batch")
        assert args[names.index("ld")] == 12 and args[names.index("sigma_px")] == 0.3
    det.localize_device(0x1000, 3, 4, 0x2000, N_IDS, 0x3000, K, None, 0.1, stream=99, cov_ptr=0x4000, sigma_px=0.3, map_cov=(0x5000, 18, 0x6000))
    names, args = last_call(det, "asl_localize_mapcov_frames_device")
    assert [value(args[names.index(n)]) for n in ("d_cov", "d_map_cov", "ld", "d_cov_slot", "stream")] == [0x4000, 0x5000, 18, 0x6000, 99]
    det.localize_rig_device(0x1000, 2, 3, 4, 0x2000, N_IDS, 0x7000, 0x3000, 0.1, stream=99, cov_ptr=0x4000, map_cov=(0x5000, 18, 0x6000))
    names, args = last_call(det, "asl_localize_rig_mapcov_frames_device")
    assert [value(args[names.index(n)]) for n in ("d_cov", "d_map_cov", "ld", "d_cov_slot", "stream")] == [0x4000, 0x5000, 18, 0x6000, 99]
    with pytest.raises(ValueError):
        det.localize(obs[0], tmap, K, None, 0.1, map_cov=cov)                       # no covariance form asked for
    with pytest.raises(ValueError):
        det.localize(obs[0], tmap, K, None, 0.1, sigma_px=0.0, map_cov=(np.zeros(3, dtype=np.int32), np.eye(12)))
    with pytest.raises(ValueError):
        det.localize_rig(obs, tmap, rig, 0.1, sigma_px=0.0, map_cov=(cov.cov_slot(N_IDS), np.eye(7)))
    assert det._L.calls == []


def test_map_covariance(tmp_path):
    M = np.arange(18.0 * 18).reshape(18, 18)
    M = M + M.T
    cov = MapCovariance.from_slots(np.array([-1, 0, -1, 1, 2, -1], dtype=np.int32), np.pad(M, ((0, 6), (0, 6))))
    assert cov.ids == [1, 3, 4] and np.array_equal(cov.matrix, M)
    assert np.array_equal(cov.block(3, 4), M[6:12, 12:18]) and np.array_equal(cov.block(4, 3), cov.block(3, 4).T)
    assert np.array_equal(cov.marginal(1), M[:6, :6]) and np.array_equal(cov.std(1), np.sqrt(np.diag(M)[:6]))
    slot, mat, ld = cov.as_args(6)
    assert slot.tolist() == [-1, 0, -1, 1, 2, -1] and slot.dtype == np.int32 and mat.flags["C_CONTIGUOUS"] and ld == 18
    assert cov.cov_slot(4).tolist() == [-1, 0, -1, 1]
    empty = MapCovariance([], np.zeros((0, 0)))
    assert empty.as_args(3)[0].tolist() == [-1, -1, -1] and empty.as_args(3)[2] == 6
    p = str(tmp_path / "cov.npz")
    cov.save_npz(p)
    back = MapCovariance.load_npz(p)
    assert back.ids == cov.ids and back.matrix.tobytes() == cov.matrix.tobytes()
    with pytest.raises(ValueError):
        MapCovariance([3, 1], np.eye(12))
    with pytest.raises(ValueError):
        MapCovariance.from_slots(np.array([1, 0]), np.eye(12))
    with pytest.raises(KeyError):
        cov.block(1, 2)
    res = np.zeros((), dtype=_lib.MAP_RESULT_DTYPE)
    r = MapResult.from_call((res, np.zeros(6, dtype=_lib.MAP_TAG_DTYPE), None, None, (slot, mat)), with_cov=True)
    assert r.cov.ids == [1, 3, 4] and r.slot_weight is None
    assert MapResult.from_call((res, None, None, None, "w")).slot_weight == "w" and MapResult.from_call((res, None, None, None)).cov is None


def test_rig_build_map_cov():
    """Rig.build_map keeps its argument list; the rig's covariance solve is Rig.build_map_cov"""
    det = detector()
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    rig = Rig([RigCamera(K), RigCamera(K)])
    r = rig.build_map_cov(det, obs, N_IDS, 0.1, world_id=3, max_iters=17)
    names, args = last_call(det, "asl_mapcov_rig_batch")
    assert args[names.index("world_id")] == 3 and args[names.index("cap_tags")] == 1 and args[names.index("tag_sizes")] is None
    assert isinstance(r, MapResult) and r.cov.ids == [] and r.slot_weight is None
    r = rig.build_map_cov(det, obs, N_IDS, 0.1, tag_sizes={3: 2.5}, huber_px=1.5)
    names, args = last_call(det, "asl_mapcov_rig_batch")
    assert args[names.index("cov_huber_px")] == 1.5 and args[names.index("tag_sizes")][3] == 2.5 and r.slot_weight is not None
