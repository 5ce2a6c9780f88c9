"""The NumPy statement of the tag-map reconstruction (tests/map_ref.py) under the Huber loss: the plain computation at huber_px 0,
the loss's gradient, the repair of corrupted slots against the plain solve, the std's variance factor, and the margins and
tolerance the device comparison (tests/test_gpu_map_robust.py) rests on."""
import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_ref as MR
import map_robust_cases as RC

K = RC.K


@pytest.mark.parametrize("case", [c[0] for c in MC.cpu_cases(K)])
def test_huber_0_is_the_plain_statement_byte_for_byte(case):
    name, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == case][0]
    want = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w)[:4]
    got = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w, huber_px=0.0)
    assert all(g.tobytes() == x.tobytes() for g, x in zip(got[:4], want))
    assert got[0]["n_soft"] == 0
    weight = got[4]
    assert set(np.unique(weight)) <= {0.0, 1.0} and weight.sum() == (want[0]["n_obs"] if want[0]["status"] == 0 else 0)
    assert not weight[obs["id"] < 0].any()


@pytest.mark.parametrize("case", ["noise", "small_slip", "dist5_swap"])
def test_a_threshold_nothing_reaches_is_the_plain_solve(case):
    obs, _, _, dist, _ = RC.repair_cases()[case]
    plain = RC.run(obs, dist, huber=0.0)
    got = RC.run(obs, dist, huber=1e6)
    assert got[0]["iterations"] == plain[0]["iterations"] and got[0]["status"] == 0 and got[0]["n_soft"] == 0
    assert np.array_equal(got[4], plain[4]) and set(np.unique(got[4])) <= {0.0, 1.0} and got[4].sum() == got[0]["n_obs"]
    assert RC.distance(got, plain) <= 1e-12


def test_gradient_of_half_the_robust_cost():
    """g is the central-difference gradient of half the robust cost at a point that is not the optimum, with corners on
    both sides of the threshold; H is symmetric"""
    obs, tags, cams, _, _ = RC.repair_cases()["small_slip"]
    table, h = MR.rig_ref.rig_table(MR.one_camera(K, None)), MR.LR.half_size(LC.TAG_INNER)
    w = int(min(i for i in obs["id"].ravel() if i >= 0))
    gt_tags, gt_cams = MC.truth(tags, cams, w)
    ids = sorted(gt_tags)
    rng = np.random.default_rng(2)

    def nudge(T):
        return MR.gn_oracle.apply_update(T, rng.normal(0, 1.0, 6) * np.array([2e-3, 2e-3, 2e-3, 0.3, 0.3, 0.3]))
    W = np.array([nudge(MR.inv(c)) for c in gt_cams])
    G = np.array([gt_tags[i] if i == w else nudge(gt_tags[i]) for i in ids])
    fs = [(f, s) for f in range(obs.shape[0]) for s in range(obs.shape[1]) if obs["id"][f, s] >= 0]
    oc = np.array([f for f, _ in fs])
    ot = np.array([ids.index(int(obs["id"][f, s])) for f, s in fs])
    ovc = np.zeros(len(fs), dtype=np.int64)
    uv = np.stack([obs["corners"][f, s].astype(np.float64).reshape(4, 2) for f, s in fs])
    cam_col = 6 * np.arange(len(W))
    tag_col = np.array([-1 if i == w else 6 * (len(W) + ids.index(i) - (ids.index(i) > ids.index(w))) for i in ids])
    npar = 6 * (len(W) + len(ids) - 1)
    over = MR.corner_terms(table, ovc, W[oc], G[ot], uv, h, RC.HUBER)[2]
    assert 0 < over.sum() < over.size

    def cost(Wx, Gx):
        return MR.joint_linearise(table, Wx, Gx, oc, ot, ovc, uv, h, cam_col, tag_col, npar, RC.HUBER)[0]
    _, H, g = MR.joint_linearise(table, W, G, oc, ot, ovc, uv, h, cam_col, tag_col, npar, RC.HUBER)
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    num = np.zeros(npar)
    eps = 1e-6
    for p in range(npar):
        for sign in (1, -1):
            d = np.zeros(npar)
            d[p] = sign * eps
            Wp, Gp = W.copy(), G.copy()
            for c in range(len(W)):
                Wp[c] = MR.gn_oracle.apply_update(W[c], d[cam_col[c]:cam_col[c] + 6])
            for j in range(len(G)):
                if tag_col[j] >= 0:
                    Gp[j] = MR.gn_oracle.apply_update(G[j], d[tag_col[j]:tag_col[j] + 6])
            num[p] += sign * 0.5 * cost(Wp, Gp) / (2 * eps)
    assert np.abs(num - g).max() <= 1e-5 * np.abs(g).max(), (np.abs(num - g).max(), np.abs(g).max())


@pytest.mark.parametrize("case", sorted(RC.ROBUST_MEASURED))
def test_errors_against_the_truth_stay_under_twice_the_recorded_ones(case):
    out, _ = RC.statement(case)
    e = RC.errors(case, out)
    print(case, "robust errors %.4g %.4g %.4g" % e, "trials", int(out[0]["iterations"]), "n_soft", int(out[0]["n_soft"]))
    assert out[0]["status"] == 0
    for got, rec in zip(e, RC.ROBUST_MEASURED[case]):
        assert got <= 2 * rec and got >= 0.5 * rec, (case, e, RC.ROBUST_MEASURED[case])   # a bar, and a record that is still true
    obs, _, _, _, bad = RC.repair_cases()[case]
    assert RC.soft_slots(obs, out) == sorted(bad + RC.EXTRA_SOFT.get(case, [])), case


@pytest.mark.parametrize("case", RC.REPAIR_ROWS)
def test_the_loss_repairs_what_wrecks_the_plain_solve(case):
    """the 12 x 24 rows: the plain solve is at least 3 x the noise-only error away, the robust one at most 1.5 x"""
    noise = RC.errors("noise", RC.statement("noise")[0])[0]
    plain = RC.errors(case, RC.statement(case, huber=0.0)[0])
    robust = RC.errors(case, RC.statement(case)[0])[0]
    print(case, "noise-only %.4g plain %.4g (%.1f x) robust %.4g (%.3f x)" % (noise, plain[0], plain[0] / noise, robust, robust / noise))
    assert all(0.5 * r <= p <= 2 * r for p, r in zip(plain, RC.PLAIN_MEASURED[case]))
    assert plain[0] >= 3 * noise
    assert robust <= 1.5 * noise


@pytest.mark.parametrize("case", ["small_slip", "small_swap"])
def test_soft_slots_are_the_corrupted_slots_on_the_small_blocks(case):
    obs, _, _, _, bad = RC.repair_cases()[case]
    out, _ = RC.statement(case)
    assert RC.soft_slots(obs, out) == bad and out[0]["n_soft"] == len(bad)
    assert all(0 < out[4][f, s] < 1 for f, s in bad)


@pytest.mark.parametrize("case", RC.REPAIR_ROWS)
def test_soft_slots_are_exactly_the_corrupted_slots(case):
    """the three 12 x 24 rows at k = 1; the noise-only row has no soft slot"""
    obs, _, _, _, bad = RC.repair_cases()[case]
    out, _ = RC.statement(case)
    soft = RC.soft_slots(obs, out)
    print(case, "soft slots", soft, "corrupted", bad)
    assert soft == bad and out[0]["n_soft"] == len(bad)
    assert RC.statement("noise")[0][0]["n_soft"] == 0


def test_the_seed_slot_swap_is_recorded_not_repaired():
    """the seed slot of frame 3 with another tag's corners and pose leaves a tag in a wrong basin: the seeding's limit.
    The figures are the baseline for later work on the seeding; the rotation stays wrong under either loss."""
    obs, tags, cams, dist, _ = RC.seed_swap_case()
    for which, huber in (("robust", RC.HUBER), ("plain", 0.0)):
        out = RC.run(obs, dist, huber=huber, with_std=False)
        e = MC.map_errors(out[1], out[3], tags, cams, int(out[0]["world_id"]))
        print(which, "errors %.4g %.4g %.4g" % e, "trials", int(out[0]["iterations"]), "n_soft", int(out[0]["n_soft"]))
        assert all(0.5 * r <= g <= 2 * r for g, r in zip(e, RC.SEED_SWAP_MEASURED[which]))


def test_one_swapped_slot_does_not_inflate_the_std():
    clean = RC.statement("noise")[0][2].max()
    robust = RC.statement("swap")[0][2].max()
    plain = RC.statement("swap", huber=0.0)[0][2].max()
    print("largest tag_std: noise-only %.4g, swap robust %.4g (%.3f x), swap plain %.4g" % (clean, robust, robust / clean, plain))
    assert 0.5 * clean <= robust <= 2 * clean
    assert plain > 2 * clean


def test_margins_tolerance_and_tails_of_the_compared_cases():
    """every compared case keeps all its corners, in every trial, at least MIN_MARGIN from the threshold; the statement
    against itself with reversed sums gives DEVICE_TOL; the trial count survives that perturbation everywhere but in
    TAIL_CASES, which are compared at COMPARE_ITERS trials"""
    worst, tails = 0.0, {}
    for name, obs, dist, iters in RC.compared_cases():
        ta, tb = {}, {}
        a = RC.run(obs, dist, trace=ta)
        b = RC.run(obs, dist, trace=tb, reverse=True)
        d = RC.distance(a, b)
        print("%-14s margin %.3g / %.3g trials %d / %d distance %.3g" % (name, ta["margin"], tb["margin"], a[0]["iterations"], b[0]["iterations"], d))
        assert a[0]["status"] == 0 and a[0]["iterations"] < RC.ITERS
        if a[0]["iterations"] != b[0]["iterations"]:
            tails[name] = d
            ta, tb = {}, {}
            a = RC.run(obs, dist, max_iters=RC.COMPARE_ITERS, trace=ta)
            b = RC.run(obs, dist, max_iters=RC.COMPARE_ITERS, trace=tb, reverse=True)
            d = RC.distance(a, b)
        assert min(ta["margin"], tb["margin"]) >= RC.MIN_MARGIN, name
        assert np.array_equal(a[4] < 1, b[4] < 1) and a[0]["n_soft"] == b[0]["n_soft"], name
        worst = max(worst, d)
    print("largest distance under reversed sums: %.3g" % worst)
    assert worst <= RC.DEVICE_TOL_MEASURED and RC.DEVICE_TOL == max(10 * RC.DEVICE_TOL_MEASURED, 1e-9)
    assert set(tails) == set(RC.TAIL_CASES)
    assert all(0.5 * RC.TAIL_CASES[n] <= d <= 2 * RC.TAIL_CASES[n] for n, d in tails.items()), tails


def test_refusals_and_the_weights_of_a_failed_solve():
    obs, _, _, dist, _ = RC.repair_cases()["small_slip"]
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            RC.run(obs, dist, huber=bad)
    ids = {int(i) for i in obs["id"].ravel() if i >= 0}
    missing = next(i for i in range(MC.N_IDS) if i not in ids)
    out = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=missing, huber_px=RC.HUBER)
    assert out[0]["status"] == 1 and out[0]["n_soft"] == 0 and not out[4].any()
