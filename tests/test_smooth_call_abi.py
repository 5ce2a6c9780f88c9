"""The one sequence-localisation call path of aprilslam_amd._lib: Detector.smooth, smooth_sequences and smooth_rig with their
device forms choose among the twelve asl_smooth* entry points by (rig, times given, huber_px, seq_start given, covariance
asked) and hand each the number of arguments its header declaration has, with the times, the offsets, huber_px and the
covariance where the declaration has them.  The entry points are stubbed on a Detector that owns no device.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from aprilslam_amd import _lib
from aprilslam_amd.rig import Rig, RigCamera
from test_smooth_cov_abi import prototype

BASES = ("asl_smooth", "asl_smooth_cov", "asl_smooth_sequences", "asl_smooth_robust_sequences", "asl_smooth_timed_sequences", "asl_smooth_rig_sequences")
ENTRIES = [b + (form if "sequences" in b else "_frames" + form if form == "_device" else form) for b in BASES for form in ("_batch", "_device")]
K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
N_IDS, N_CAMS, N, MT = 8, 2, 5, 4
START = [0, 2, 5]
HUBER = 1.5
SIGMAS = (0.5, 0.01, 0.2)


def entry(rig, times, huber, seq, cov):
    """the routing table of Detector._smooth_call"""
    if rig:
        return "asl_smooth_rig_sequences"
    if times:
        return "asl_smooth_timed_sequences"
    if huber:
        return "asl_smooth_robust_sequences"
    if seq:
        return "asl_smooth_sequences"
    return "asl_smooth_cov" if cov else "asl_smooth"


ROWS = list(itertools.product((False, True), repeat=5))       # (rig, times given, huber_px != 0, seq_start given, cov asked)


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


def null(a):
    return not (a if isinstance(a, C._Pointer) else value(a))


def check_call(det, want, row, device):
    rig, times, huber, seq, cov = row
    (name, args), = det._L.calls
    det._L.calls.clear()
    names = prototype(name)
    assert name == want and len(args) == len(names), (name, want, len(args), len(names))
    hub = [i for i, n in enumerate(names) if "huber" in n]
    assert len(hub) == (1 if any(k in name for k in ("robust", "timed", "rig")) else 0)
    if hub:
        assert type(args[hub[0]]) is float and args[hub[0]] == (HUBER if huber else 0.0) and names[hub[0] - 1] == "sigma_trans"
    else:
        assert not huber
    tm = [i for i, n in enumerate(names) if "times" in n]
    assert len(tm) == (1 if rig or times else 0)
    if tm:
        assert null(args[tm[0]]) == (not times) and names[tm[0] - 1] in ("seed", "d_seed")
        if times:
            assert value(args[tm[0]]) == 0x8000 if device else [args[tm[0]][i] for i in range(N)] == [10.0, 11.0, 12.5, 13.0, 14.0]
    if "seq_start" in names:
        i = names.index("seq_start")
        start = START if seq else [0, N]
        assert names[i + 1] == "n_seq" and args[i + 1] == len(start) - 1 and [args[i][k] for k in range(len(start))] == start
    else:
        assert not seq and "n_seq" not in names
    cv = [i for i, n in enumerate(names) if n in ("cov", "d_cov")]
    assert len(cv) == (0 if name.startswith(("asl_smooth_batch", "asl_smooth_frames")) else 1)
    if cv:
        assert null(args[cv[0]]) == (not cov) and cv[0] == len(names) - (2 if device else 1)
    else:
        assert not cov
    assert args[names.index("max_iters")] == 17 and args[names.index("n_ids")] == N_IDS and args[names.index("n_frames")] == N
    assert [args[names.index(k)] for k in ("sigma_px", "sigma_rot", "sigma_trans")] == list(SIGMAS)
    assert ("n_cams" in names) == rig and (not rig or args[names.index("n_cams")] == N_CAMS)
    if device:
        assert names[-1] == "stream" and value(args[-1]) == 99


@pytest.mark.parametrize("row", ROWS, ids=["rig%d_times%d_huber%d_seq%d_cov%d" % r for r in ROWS])
def test_the_entry_point_and_its_arguments(row):
    rig, times, huber, seq, cov = row
    want = entry(*row)
    det = detector()
    obs = np.zeros((N_CAMS, N, MT), dtype=_lib.OBS_DTYPE)
    tag_map, seed = np.zeros(N_IDS, dtype=_lib.MAP_TAG_DTYPE), np.zeros(N, dtype=_lib.CAM_POSE_DTYPE)
    kw = dict(max_iters=17, huber_px=HUBER if huber else 0.0)
    host = dict(kw, seed=seed, with_cov=cov, times=np.array([10.0, 11.0, 12.5, 13.0, 14.0]) if times else None)
    dev = dict(kw, stream=99, cov_ptr=0x7000 if cov else None, times_ptr=0x8000 if times else None)
    if rig:
        out = det.smooth_rig(obs, tag_map, Rig([RigCamera(K), RigCamera(K)]), 0.1, *SIGMAS, seq_start=START if seq else None, **host)
    elif seq:
        out = det.smooth_sequences(obs[0], START, tag_map, K, None, 0.1, *SIGMAS, **host)
    else:
        out = det.smooth(obs[0], tag_map, K, None, 0.1, *SIGMAS, **host)
    assert len(out) == (3 if cov else 2) and out[0].shape == (N,) and out[0].dtype == _lib.CAM_POSE_DTYPE
    assert out[1].shape == ((len(START) - 1,) if seq else ()) and out[1].dtype == _lib.SMOOTH_RESULT_DTYPE
    assert not cov or (out[2].shape == (N,) and out[2].dtype == _lib.POSE_COV_DTYPE)
    check_call(det, want + "_batch", row, False)
    if rig:
        got = det.smooth_rig_device(0x1000, N_CAMS, N, MT, 0x2000, N_IDS, 0x6000, 0x3000, 0x4000, 0x5000, 0.1, *SIGMAS, seq_start=START if seq else None, **dev)
    elif seq:
        got = det.smooth_sequences_device(0x1000, N, MT, 0x2000, N_IDS, 0x3000, START, 0x4000, 0x5000, K, None, 0.1, *SIGMAS, **dev)
    else:
        got = det.smooth_device(0x1000, N, MT, 0x2000, N_IDS, 0x3000, 0x4000, 0x5000, K, None, 0.1, *SIGMAS, **dev)
    assert got is None
    check_call(det, want + ("_device" if "sequences" in want else "_frames_device"), row, True)


def test_the_stubbed_names_are_the_twelve_exports():
    assert len(ENTRIES) == 12 and sorted(ENTRIES) == sorted(n for n in _lib.EXPORTS if n.startswith("asl_smooth"))


def test_argument_checks_come_before_any_call():
    det = detector()
    obs = np.zeros((N_CAMS, N, MT), dtype=_lib.OBS_DTYPE)
    tag_map, seed = np.zeros(N_IDS, dtype=_lib.MAP_TAG_DTYPE), np.zeros(N, dtype=_lib.CAM_POSE_DTYPE)
    pair = Rig([RigCamera(K), RigCamera(K)])
    for call in (lambda: det.smooth(obs, tag_map, K, None, 0.1),                                        # obs rank
                 lambda: det.smooth(obs[0], tag_map, np.eye(2), None, 0.1),                              # K
                 lambda: det.smooth(obs[0], tag_map, K, None, 0.1, seed=seed[:-1]),                      # seed length
                 lambda: det.smooth(obs[0], tag_map, K, None, 0.1, times=np.arange(N + 1.0)),            # times length
                 lambda: det.smooth_sequences(obs[0], START, tag_map, K, None, 0.1, seed=seed[:-1]),
                 lambda: det.smooth_sequences(obs[0], START, tag_map, K, None, 0.1, times=np.arange(N + 1.0)),
                 lambda: det.smooth_rig(obs[0], tag_map, pair, 0.1),                                     # obs rank
                 lambda: det.smooth_rig(obs, tag_map, Rig([RigCamera(K)]), 0.1),                         # rig size
                 lambda: det.smooth_rig(obs, tag_map, pair, 0.1, seed=seed[:-1]),
                 lambda: det.smooth_rig(obs, tag_map, pair, 0.1, times=np.arange(N + 1.0))):
        with pytest.raises(ValueError):
            call()
    assert det._L.calls == []
