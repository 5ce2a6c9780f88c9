"""The one map call path of aprilslam_amd._lib: Detector.build_map, build_map_device, build_map_rig and build_map_rig_device
choose among the ten asl_map_* entry points by (rig, tag_sizes given, huber_px or weights asked) and hand each the number
of arguments its header declaration has, with tag_sizes, huber_px and the slot weights where the declaration has them.  The
entry points are stubbed on a Detector that owns no device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from aprilslam_amd import _lib
from aprilslam_amd.rig import Rig, RigCamera
from test_smooth_cov_abi import prototype

ENTRIES = [base + form for base in ("asl_map", "asl_map_robust", "asl_map_sized", "asl_map_rig", "asl_map_rig_sized") for form in ("_batch", "_frames_device")]
K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
N_IDS = 8
# (tag_sizes given, huber_px, weights asked) -> the entry of one camera, of a rig
TABLE = [((False, 0.0, False), "asl_map", "asl_map_rig"),
         ((False, 1.5, False), "asl_map_robust", "asl_map_rig"),
         ((False, 0.0, True), "asl_map_robust", "asl_map_rig"),
         ((False, 1.5, True), "asl_map_robust", "asl_map_rig"),
         ((True, 0.0, False), "asl_map_sized", "asl_map_rig_sized"),
         ((True, 1.5, False), "asl_map_sized", "asl_map_rig_sized"),
         ((True, 0.0, True), "asl_map_sized", "asl_map_rig_sized"),
         ((True, 1.5, True), "asl_map_sized", "asl_map_rig_sized")]


class Stub:
    """records (entry, arguments) of every call and returns 0"""

    def __init__(self):
        self.calls = []
        for name in ENTRIES:
            setattr(self, name, lambda *a, _n=name: self.calls.append((_n, a)) or 0)


def detector():
    det = object.__new__(_lib.Detector)
    det._L, det._h = Stub(), C.c_void_p(1)
    return det


def value(a):
    return a.value if isinstance(a, C.c_void_p) else a


def check_call(det, entry, sized, huber, weight_given, device):
    (name, args), = det._L.calls
    det._L.calls.clear()
    names = prototype(name)
    assert name == entry and len(args) == len(names), (name, len(args), len(names))
    assert ("tag_sizes" in names) == sized
    if sized:
        t = args[names.index("tag_sizes")]
        assert isinstance(t, C.POINTER(C.c_float)) and [t[i] for i in range(N_IDS)] == [0, 0, 0, 2.5, 0, 0, 0, 0]
    hub = [i for i, n in enumerate(names) if n.endswith("huber_px")]
    assert len(hub) == (0 if entry.startswith("asl_map_batch") or entry.startswith("asl_map_frames") else 1)
    if hub:
        assert args[hub[0]] == huber and type(args[hub[0]]) is float
        w = value(args[-2 if device else -1])
        assert (w is not None and w != 0) == weight_given
    else:
        assert not huber and not weight_given
    assert args[names.index("max_iters")] == 17 and args[names.index("world_id")] == 3 and args[names.index("n_ids")] == N_IDS
    if device:
        assert names[-1] == "stream" and value(args[-1]) == 99


@pytest.mark.parametrize("row", TABLE, ids=[str(r[0]) for r in TABLE])
def test_the_entry_point_and_its_argument_count(row):
    (sized, huber, weights), cam_entry, rig_entry = row
    sizes = {3: 2.5} if sized else None
    det = detector()
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    rig = Rig([RigCamera(K), RigCamera(K)])
    out = det.build_map(obs[0], N_IDS, K, None, 0.1, world_id=3, max_iters=17, huber_px=huber, with_slot_weight=weights, tag_sizes=sizes)
    assert len(out) == (5 if weights else 4) and out[1].shape == (N_IDS,) and out[3].shape == (3,) and (not weights or out[4].shape == (3, 4))
    check_call(det, cam_entry + "_batch", sized, huber, weights, False)
    out = det.build_map_rig(obs, N_IDS, rig, 0.1, world_id=3, max_iters=17, huber_px=huber, with_slot_weight=weights, tag_sizes=sizes)
    assert len(out) == (5 if weights else 4) and out[3].shape == (3,) and (not weights or out[4].shape == (2, 3, 4))
    check_call(det, rig_entry + "_batch", sized, huber, weights, False)
    wp = 0x7000 if weights else 0
    assert det.build_map_device(0x1000, 3, 4, N_IDS, K, None, 0.1, 0x2000, 0, 0x4000, 0x5000, world_id=3, max_iters=17, stream=99, huber_px=huber,
                                slot_weight_ptr=wp, tag_sizes=sizes) is None
    check_call(det, cam_entry + "_frames_device", sized, huber, weights, True)
    assert det.build_map_rig_device(0x1000, 2, 3, 4, N_IDS, 0x6000, 0.1, 0x2000, 0x3000, 0x4000, 0x5000, world_id=3, max_iters=17, stream=99,
                                    huber_px=huber, slot_weight_ptr=wp, tag_sizes=sizes) is None
    check_call(det, rig_entry + "_frames_device", sized, huber, weights, True)


def test_the_stubbed_names_are_the_ten_exports():
    assert sorted(ENTRIES) == sorted(n for n in _lib.EXPORTS if n.startswith("asl_map_"))


def test_argument_checks_come_before_any_call():
    det = detector()
    obs = np.zeros((2, 3, 4), dtype=_lib.OBS_DTYPE)
    with pytest.raises(ValueError):
        det.build_map(obs[0], N_IDS, np.eye(2), None, 0.1)
    with pytest.raises(ValueError):
        det.build_map(obs[0], N_IDS, K, np.zeros(3), 0.1)
    with pytest.raises(ValueError):
        det.build_map_rig(obs[0], N_IDS, Rig([RigCamera(K)]), 0.1)
    with pytest.raises(ValueError):
        det.build_map_rig(obs, N_IDS, Rig([RigCamera(K)]), 0.1)
    with pytest.raises(ValueError):
        det.build_map(obs[0], N_IDS, K, None, 0.1, tag_sizes=np.zeros(N_IDS + 1))
    assert det._L.calls == []
