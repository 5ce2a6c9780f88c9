"""The NumPy statement of the tag-map reconstruction (tests/map_ref.py) with a size table: an all-zero table is no table to the
byte, one camera at the identity against the single-camera front, the truth on exact data, that every entry of the device comparison's list
happens in its cases (through the statement's trace), and the recorded figures of tests/map_sized_cases.py measured again."""
import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_ref as MR
import map_rig_cases as GC
import map_sized_cases as ZC
import sized_cases as SC
from aprilslam_amd.rig import Rig, RigCamera

INTS = ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft")


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["slots_3x5", "slots_1x17", "list_16_17", "behind", "repeated_id"])
def test_an_all_zero_table_is_the_rig_statement_to_the_byte(name):
    """the rig statement: the call without a table"""
    obs, rig = GC.edge_cases()[name]
    for huber, reverse in ((0.0, False), (GC.HUBER, False), (GC.HUBER, True)):
        want = MR.map_rig_frames(obs, GC.N_IDS, rig, GC.TAG, huber_px=huber, max_iters=20, reverse=reverse)
        for t in (None, np.zeros(GC.N_IDS, dtype=np.float32)):
            assert same_bytes(MR.map_rig_frames(obs, GC.N_IDS, rig, GC.TAG, t, huber_px=huber, max_iters=20, reverse=reverse), want), (name, huber, reverse)


@pytest.mark.parametrize("case", [c[0] for c in MC.cpu_cases(MC.K_bench())])
def test_one_camera_at_the_identity_is_the_single_camera_statement(case):
    """Everything map_rig_frames returns for the camera without a table, byte for byte, and with it map_frames' map and
    poses byte for byte, its integers, and its cost and std to the last bits (the bounds of the time when map_frames
    summed the cost over all corners at once and differed there; it is the same computation now)."""
    K = MC.K_bench()
    _, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == case][0]
    solo = Rig([RigCamera(K, dist, np.eye(4))])
    got = MR.map_rig_frames(obs[None], MC.N_IDS, solo, LC.TAG_INNER, np.zeros(MC.N_IDS, dtype=np.float32), world_id=w)
    assert same_bytes(got, MR.map_rig_frames(obs[None], MC.N_IDS, solo, LC.TAG_INNER, world_id=w))
    want = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w)
    assert got[1].tobytes() == want[1].tobytes() and got[3].tobytes() == want[3].tobytes(), case
    assert all(got[0][k] == want[0][k] for k in INTS)
    assert abs(got[0]["cost"] - want[0]["cost"]) <= 4 * np.spacing(want[0]["cost"])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-14, atol=0)


def test_bad_entries_are_refused():
    obs, rig, t = ZC.edge_cases()["behind"]
    for bad in (-1.0, np.nan, np.inf):
        tt = t.copy()
        tt[7] = bad
        with pytest.raises(ValueError, match=r"tag_sizes\[7\]"):
            ZC.run(obs, rig, tt)


def test_truth():
    """exact corners and records: the statement finds the truth with the table, and without it puts tag 5 at the wrong
    distance"""
    obs, t, gt, gp = ZC.truth_case()
    base, bar = ZC.truth_bar()
    out = MR.map_rig_frames(obs, 6, SC.one_camera(), ZC.TAG, t, max_iters=ZC.ITERS)
    plain = MR.map_rig_frames(obs, 6, SC.one_camera(), ZC.TAG, None, max_iters=ZC.ITERS)
    e, ep = ZC.truth_err(out, gt, gp), ZC.truth_err(plain, gt, gp)
    print("truth: sized %.3g, equal sizes %.3g (bar %.3g), without the table %.3g" % (e, base, bar, ep))
    assert out[0]["status"] == 0 and out[0]["n_tags"] == 6 and e <= bar
    assert np.array_equal(out[1]["size"], t) and not plain[1]["size"].any()
    for got, name in ((e, "sized"), (base, "equal"), (ep, "plain")):
        assert abs(got - ZC.TRUTH_ERRORS[name]) <= 1e-2 * ZC.TRUTH_ERRORS[name], (name, got)


def test_a_table_of_the_tag_size_changes_the_size_field_alone():
    obs, rig, _ = ZC.main_cases()["pair_mixed"]
    a = ZC.run(obs, rig, None, max_iters=10)
    b = ZC.run(obs, rig, np.full(ZC.N_IDS, ZC.TAG, dtype=np.float32), max_iters=10)
    assert same_bytes((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4]))
    assert a[1]["T"].tobytes() == b[1]["T"].tobytes() and np.array_equal(b[1]["size"], np.where(b[1]["valid"], np.float32(ZC.TAG), 0))


def test_the_cases_hold_what_they_are_for():
    """every entry of the device comparison's list, seen in the statement's trace"""
    main, edge = ZC.main_cases(), ZC.edge_cases()
    tr = {}
    obs, rig, t = main["pair_mixed"]
    out = ZC.run(obs, rig, t, trace=tr)
    sized = set(np.flatnonzero(t > 0).tolist())
    ratios = {float(t[i]) / ZC.TAG for i in np.flatnonzero(out[1]["valid"]) if t[i] > 0}
    assert min(ratios) == 0.25 and max(ratios) == 4.0 and len(ratios) == len(ZC.RATIOS)          # mixed sizes across RATIOS
    assert out[0]["world_id"] == 0 and t[0] > 0                                                  # a sized world tag
    assert any(i in sized for _, i in tr["chain_frames"]) and any(j in sized for j in tr["chain_tags"])
    assert any(not t[j] for j in tr["chain_tags"])                                               # and tags without a size
    assert t[40:].all() and not out[1]["valid"][40:].any() and not out[1]["size"][40:].any()     # entries for ids never seen
    assert np.array_equal(out[1]["size"], np.where(out[1]["valid"], t, 0))
    both = [(f, int(i)) for f in range(obs.shape[1]) for i in obs["id"][0, f] if i in sized and i in obs["id"][1, f]]
    assert both and tr["pairs"] < tr["views"]                                                    # the same sized id in both cameras
    tr = {}
    obs, rig, t = edge["mirrored_sweep"]
    ZC.run(obs, rig, t, trace=tr)
    assert any(w[0] == "frame" and w[1] == 2 and t[w[2]] > 0 for w in tr["sweep_mirrored"]), tr["sweep_mirrored"]
    assert any(f == 2 and t[i] > 0 for f, i in tr["chain_frames"])
    tr = {}
    obs, rig, t = edge["flip"]
    ZC.run(obs, rig, t, trace=tr)
    assert tr["flipped"] == [ZC.FLIP_TAG] and t[ZC.FLIP_TAG] == 2 * ZC.TAG
    tr = {}
    obs, rig, t = edge["behind"]
    out = ZC.run(obs, rig, t, trace=tr)
    assert tr["behind"] == [2] and t[2] > 0 and out[0]["n_obs_dropped"] == 1 and out[3]["n_rejected"][1] == 1 and out[1]["valid"][2]
    obs, rig, t = edge["all_sized"]
    assert all(t[i] > 0 for i in np.unique(obs["id"]) if i >= 0)
    for (nc, mt), slots in (((3, 5), 15), ((2, 8), 16), ((1, 17), 17)):
        obs, rig, t = edge["slots_%dx%d" % (nc, mt)]
        assert obs.shape == (nc, 4, mt) and nc * mt == slots and (obs["id"][:, 0] >= 0).all()
        assert t[obs["id"][nc - 1, 0, mt - 1]] == 2 * ZC.TAG                                     # 1 x 17: global slot 16
    obs, rig, t = edge["list_16_17"]
    assert (obs["id"] == 3).sum() == 16 and (obs["id"] == 4).sum() == 17 and t[3] > 0 and t[4] > 0
    for obs, _, _ in list(main.values()) + list(edge.values()):
        assert obs.shape[1] <= 12 and obs.shape[2] <= 24


def test_the_device_comparison_rests_on_these():
    """the reversal distances, the tail cases and the margins of every compared case, measured again; no main case is a tail
    case and at most a quarter of the edge cases are"""
    worst = 0.0
    assert not any(n in ZC.main_cases() for n, _ in ZC.TAIL_CASES) and 4 * len(ZC.TAIL_CASES) <= 2 * len(ZC.edge_cases())
    for name, obs, rig, t, huber, iters in ZC.compared_cases():
        tr = {}
        a, b = ZC.run(obs, rig, t, huber, iters, trace=tr), ZC.run(obs, rig, t, huber, iters, reverse=True)
        assert a[0]["status"] == 0 and all(a[0][k] == b[0][k] for k in INTS), (name, huber)
        worst = max(worst, ZC.distance(a, b))
        if huber > 0:
            assert tr["margin"] >= ZC.MIN_MARGIN, (name, tr["margin"])
        if (name, huber) in ZC.TAIL_CASES:
            ca, cb = ZC.run(obs, rig, t, huber), ZC.run(obs, rig, t, huber, reverse=True)
            assert ca[0]["iterations"] != cb[0]["iterations"] and max(ca[0]["iterations"], cb[0]["iterations"]) < ZC.ITERS
            d = ZC.distance(ca, cb)
            assert d <= 1.05 * ZC.TAIL_CASES[(name, huber)], (name, huber, d)
    print("largest reversal distance %.3g" % worst)
    assert worst <= 1.05 * ZC.DEVICE_TOL_MEASURED
