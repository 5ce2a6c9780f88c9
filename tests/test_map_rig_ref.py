"""The NumPy statement of the tag-map reconstruction (tests/map_ref.py) on a camera rig: one camera at the identity against the
single-camera front, the LM's gradient with a mounting, the fold of a pair's views, the split, overlap and swapped-slot
cases with their recorded figures, and the measurements the device comparison (tests/test_gpu_map_rig.py) rests on."""
import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import map_cases as MC
import map_ref as MR
import map_rig_cases as GC
import map_robust_cases as RBC
import rig_ref
from aprilslam_amd.mapping import MapResult
from aprilslam_amd.rig import Rig, RigCamera

K = MC.K_bench()
INTS = ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft")


@pytest.mark.parametrize("case", [c[0] for c in MC.cpu_cases(K)])
def test_one_camera_at_the_identity_is_the_single_camera_statement(case):
    """integer fields equal, doubles under the device's bound (not bytes: the arithmetic is ordered differently)"""
    _, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == case][0]
    solo = Rig([RigCamera(K, dist, np.eye(4))])
    for huber in (0.0, RBC.HUBER):
        want = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w, huber_px=huber)
        got = MR.map_rig_frames(obs[None], MC.N_IDS, solo, LC.TAG_INNER, world_id=w, huber_px=huber)
        for k in INTS:
            assert got[0][k] == want[0][k], (case, huber, k)
        for k in ("status", "n_tags", "n_rejected", "seed_slot"):
            assert np.array_equal(got[3][k], want[3][k]), (case, huber, k)
        assert np.array_equal(got[1]["valid"], want[1]["valid"])
        assert GC.distance(got, want) <= GC.DEVICE_TOL, (case, huber, GC.distance(got, want))
        assert np.abs(got[4][0] - want[4]).max() <= GC.DEVICE_TOL
        np.testing.assert_allclose(got[2], want[2], rtol=1e-6, atol=1e-12)
        if huber == 0.0 and w == -1:
            plain = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[:4], want[:4]))


def small_problem():
    """12 views of a mixed-model rig with mountings that are not the identity: (table, W, G, oc, ot, ovc, uv, h)"""
    obs = GC.mixed_block(GC.NOISE)[:, :3]
    table = rig_ref.rig_table(GC.MIXED)
    tm = GC.scene()
    poses = GC.bench_poses(3)
    ids = [0, 1, 2, 3]
    views = [(f, i, c, int(np.flatnonzero(obs["id"][c, f] == i)[0])) for f in range(3) for c in range(2) for i in ids if i in obs["id"][c, f]]
    rng = np.random.default_rng(2)
    W = np.array([MR.gn_oracle.apply_update(MR.inv(T), rng.normal(size=6) * 0.01) for T in poses])
    G = np.array([MR.gn_oracle.apply_update(tm[i], rng.normal(size=6) * 0.01) for i in ids])
    oc = np.array([v[0] for v in views])
    ot = np.array([ids.index(v[1]) for v in views])
    ovc = np.array([v[2] for v in views])
    uv = np.stack([obs["corners"][c, f, s].astype(np.float64).reshape(4, 2) for f, _, c, s in views])
    assert len({(a, b) for a, b in zip(oc, ot)}) < len(views)          # some pair has two views
    return table, W, G, oc, ot, ovc, uv, LR.half_size(GC.TAG)


@pytest.mark.parametrize("huber", [0.0, 1.0])
def test_gradient_is_the_central_difference_of_half_the_cost(huber):
    table, W, G, oc, ot, ovc, uv, h = small_problem()
    cam_col, tag_col = 6 * np.arange(3), 18 + 6 * np.arange(4)
    _, H, g = MR.joint_linearise(table, W, G, oc, ot, ovc, uv, h, cam_col, tag_col, 42, huber)

    def cost(x):
        Wx = np.array([MR.gn_oracle.apply_update(W[c], x[6 * c:6 * c + 6]) for c in range(3)])
        Gx = np.array([MR.gn_oracle.apply_update(G[j], x[18 + 6 * j:24 + 6 * j]) for j in range(4)])
        return MR.joint_linearise(table, Wx, Gx, oc, ot, ovc, uv, h, cam_col, tag_col, 42, huber)[0]

    num = np.zeros(42)
    for i in range(42):
        d = np.zeros(42)
        d[i] = 1e-6
        num[i] = (cost(d) - cost(-d)) / 4e-6
    assert np.abs(num - g).max() <= 1e-6 * np.abs(g).max(), np.abs(num - g).max() / np.abs(g).max()


def test_the_fold_leaves_the_normal_matrix_alone():
    table, W, G, oc, ot, ovc, uv, h = small_problem()
    cam_col, tag_col = 6 * np.arange(3), 18 + 6 * np.arange(4)
    tag_col[0] = -1                                              # a held tag, as the world tag is
    ca, Ha, ga = MR.joint_linearise(table, W, G, oc, ot, ovc, uv, h, cam_col, tag_col, 42, fold=False)
    tr = {}
    cb, Hb, gb = MR.joint_linearise(table, W, G, oc, ot, ovc, uv, h, cam_col, tag_col, 42, trace=tr, fold=True)
    assert tr["pairs"] < tr["views"] == len(oc) and ca == cb
    assert np.abs(Ha - Hb).max() <= 1e-12 * np.abs(Ha).max() and np.abs(ga - gb).max() <= 1e-12 * np.abs(ga).max()


def test_split_case():
    exact = GC.split(GC.pair_block(12, 24))
    a0, a1 = GC.single(exact, 0), GC.single(exact, 1)
    assert (a0[0]["n_tags"], a0[0]["world_id"], a1[0]["n_tags"], a1[0]["world_id"]) == (9, 0, 8, 10)
    assert GC.single(exact, 1, world_id=0)[0]["status"] == 1       # no common gauge: camera 1 never sees tag 0
    r = GC.run(exact, GC.PAIR, max_iters=30)
    assert r[0]["status"] == 0 and r[0]["n_tags"] == 17 and r[0]["n_frames_used"] == 12
    noisy, rig = GC.main_cases()["split"]
    poses = GC.bench_poses(12)
    er = GC.truth_errors(GC.run(noisy, rig), poses)[0]
    e0, e1 = GC.truth_errors(GC.single(noisy, 0), poses)[0], GC.truth_errors(GC.single(noisy, 1), poses)[0]
    print("split at %.1f px: rig %.4g, camera 0 %.4g, camera 1 %.4g" % (GC.NOISE, er, e0, e1))
    assert er <= 1.5 * max(e0, e1)
    for got, name in ((er, "rig"), (e0, "camera0"), (e1, "camera1")):
        assert abs(got - GC.SPLIT_ERRORS[name]) <= 1e-3 * GC.SPLIT_ERRORS[name], (name, got)


def mean_std(out):
    v = np.flatnonzero(out[1]["valid"])
    return float(out[2][v[v != int(out[0]["world_id"])]].mean())


def test_overlap_case():
    obs, rig = GC.main_cases()["overlap"]
    assert GC.view_counts(obs) == (392, 240)
    tr = {}
    a, b = GC.run(obs, rig, trace=tr), GC.run(GC.one_view_per_pair(obs), rig)
    assert (tr["views"], tr["pairs"]) == (392, 240) and a[0]["n_obs"] == 392 and b[0]["n_obs"] == 240
    print("overlap: mean tag std %.4g with every view, %.4g with one view per pair" % (mean_std(a), mean_std(b)))
    assert mean_std(a) < mean_std(b)
    assert abs(mean_std(a) - GC.OVERLAP_STD["all_views"]) <= 1e-3 and abs(mean_std(b) - GC.OVERLAP_STD["one_per_pair"]) <= 1e-3


def test_mixed_models_reach_the_same_quality():
    obs, rig = GC.main_cases()["mixed_models"]
    out = GC.run(obs, rig)
    et = GC.truth_errors(out, GC.bench_poses(12))[0]
    print("mixed models: largest tag translation error %.4g, rms %.4g px" % (et, out[0]["rms_px"]))
    assert out[0]["status"] == 0 and out[0]["n_tags"] == 20 and out[0]["rms_px"] < 1.5 * GC.NOISE * np.sqrt(2) and et < 2.5


def test_swapped_slot_in_camera_1():
    obs, rig = GC.main_cases()["overlap"]
    sw = GC.swap_slot(obs, *GC.SWAPPED)
    poses = GC.bench_poses(12)
    tr = {}
    plain, robust = GC.run(sw, rig), GC.run(sw, rig, huber=GC.HUBER, trace=tr)
    ep, er = GC.truth_errors(plain, poses)[0], GC.truth_errors(robust, poses)[0]
    print("swapped slot: plain %.4g, robust %.4g" % (ep, er))
    assert ep >= 3 * er and tr["margin"] >= GC.MIN_MARGIN
    assert abs(ep - GC.SWAP_ERRORS["plain"]) <= 1e-2 * GC.SWAP_ERRORS["plain"] and abs(er - GC.SWAP_ERRORS["robust"]) <= 1e-3
    soft = [t[:3] for t in MapResult(*robust[:4], slot_weight=robust[4], slot_ids=sw["id"]).soft_slots()]
    assert sorted(soft) == sorted([GC.SWAPPED] + GC.EXTRA_SOFT) and robust[0]["n_soft"] == len(soft)


def test_the_device_comparison_rests_on_these():
    """the reversal distances, the tail cases and the margins of every compared case, measured again"""
    worst = 0.0
    for name, obs, rig, huber, iters in GC.compared_cases():
        tr = {}
        a, b = GC.run(obs, rig, huber=huber, max_iters=iters, trace=tr), GC.run(obs, rig, huber=huber, max_iters=iters, reverse=True)
        assert a[0]["status"] == 0 and all(a[0][k] == b[0][k] for k in INTS), (name, huber)
        worst = max(worst, GC.distance(a, b))
        if huber > 0:
            assert tr["margin"] >= GC.MIN_MARGIN, (name, tr["margin"])
        if (name, huber) in GC.TAIL_CASES:
            ca, cb = GC.run(obs, rig, huber=huber), GC.run(obs, rig, huber=huber, reverse=True)
            assert ca[0]["iterations"] != cb[0]["iterations"] and max(ca[0]["iterations"], cb[0]["iterations"]) < GC.ITERS
            d = GC.distance(ca, cb)
            assert d <= 1.05 * GC.TAIL_CASES[(name, huber)], (name, huber, d)
    print("largest reversal distance %.3g" % worst)
    assert worst <= 1.05 * GC.DEVICE_TOL_MEASURED
