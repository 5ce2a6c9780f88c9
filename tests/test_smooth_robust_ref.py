"""The robust (huber_px > 0) path of the NumPy statement of the sequence localisation (tests/smooth_ref.py) on the CPU: that
its plain path stands on the localisation's statement and its weighted path with every weight 1 agrees with it, that its
weighted sums are the derivatives of the loss it states, that the cases of tests/smooth_robust_cases.py exercise both
branches of the loss, and that the figures recorded there still hold."""
import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_robust_cases as RC
import smooth_ref as SR
import smooth_seq_cases as SQ
import solver_checks as CK

SHAPE_NAMES = ["shape%d_%d_%d" % s for s in RC.SHAPES]


@pytest.mark.parametrize("name", [c[0] for c in SC.all_cases()])
def test_huber_zero_is_the_plain_statement(name):
    """huber_px 0 given explicitly is the call without it; the two tests below say what the plain path stands on"""
    _, obs, rec, seed, dist, sig, iters = [c for c in SC.all_cases() if c[0] == name][0]
    want, wres, wtrace = SC.statement(name)
    got, res, trace = SR.smooth(obs, rec, SC.K, dist, SC.TAG, seed, *sig, iters, huber_px=0.0)
    assert got.tobytes() == want.tobytes() and res.tobytes() == wres.tobytes()
    assert np.array_equal(trace["choice"], wtrace["choice"]) and res["n_soft"] == 0 and not got["n_rejected"].any()


@pytest.mark.parametrize("name", [c[0] for c in SC.all_cases()])
def test_plain_path_is_the_localisation_statement(name):
    """huber_px 0: every frame's c, H, g of every linearisation (the chain's and each trial's) are the bytes of
    localize_ref.linearise at that pose; no soft slot anywhere"""
    out, res, trace = SC.statement(name)
    pb = trace["problem"]
    assert pb.k == 0.0 and res["n_soft"] == 0 and not out["n_rejected"].any()
    assert len(trace["lins"]) >= 1 or res["status"] == SR.NO_POSED_FRAME
    for P, lin in trace["lins"]:
        assert not lin["soft"].any()
        for f in range(pb.n):
            c, H, g = (0.0, np.zeros((6, 6)), np.zeros(6)) if pb.pts[f] is None else LR.linearise(pb.model.cam, P[f][0], P[f][1], *pb.pts[f][:2])
            assert np.float64(c).tobytes() == lin["c"][f].tobytes() and H.tobytes() == lin["H"][f].tobytes() and g.tobytes() == lin["g"][f].tobytes()


# flips and flips_first: their trial counts hang on a rounding (14 against 9 and 10 against 12 trials between the two paths)
ALL_WEIGHTS_ONE = [c[0] for c in SC.all_cases() if c[0] not in ("flips", "flips_first")]


@pytest.mark.parametrize("name", ALL_WEIGHTS_ONE)
def test_weighted_path_with_all_weights_one(name):
    """at a threshold no corner reaches the weighted path runs with every weight 1: the plain run's status and trials, no
    soft slot, every T within ROBUST_TOL of the plain statement's"""
    _, obs, rec, seed, dist, sig, iters = [c for c in SC.all_cases() if c[0] == name][0]
    want, wres, _ = SC.statement(name)
    got, res, trace = SC.run(obs, rec, seed, dist, sig, max_iters=iters, huber=1e9)
    assert trace["problem"].k == 1e9 and res["status"] == wres["status"] and res["iterations"] == wres["iterations"]
    assert res["n_soft"] == 0 and not got["n_rejected"].any()
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d" % (name, worst, RC.ROBUST_TOL, res["iterations"]))
    assert worst <= RC.ROBUST_TOL, (name, worst)


def rho_sum(pb, f, P):
    return float(SR.corner_terms(pb.model, P[0], P[1], *pb.pts[f], pb.k)[0].sum())


@pytest.mark.parametrize("name", ["shape3_4_0", "shape5_20_5", "shape1_1_0"])
def test_h_and_g_are_the_weighted_sums(name):
    """g = sum wgt J^T r is half the gradient of sum rho (central differences of the stated loss along the left update), H =
    sum wgt J^T J, both against sums written corner by corner; the cost is sum rho"""
    _, _, trace = RC.statement(name)
    pb = trace["problem"]
    P, lin = trace["lins"][0]
    for f in range(pb.n):
        if pb.pts[f] is None:
            continue
        c, H, g, soft, wgt, s = pb.frame(f, P[f])
        assert (wgt < 1).any() == (soft > 0) and c == rho_sum(pb, f, P[f]) and c == lin["c"][f]
        assert np.array_equal(H, lin["H"][f]) and np.array_equal(g, lin["g"][f]) and soft == lin["soft"][f]
        # corner by corner
        Xw, uv, ci = pb.pts[f]
        Hs, gs = np.zeros((6, 6)), np.zeros(6)
        for i in range(len(Xw)):
            _, w1, _, ok, J, r = SR.corner_terms(pb.model, P[f][0], P[f][1], Xw[i:i + 1], uv[i:i + 1], ci[i:i + 1], pb.k, jac=True)
            assert ok[0]
            over = s[i] > pb.k
            assert w1[0] == (pb.k / s[i] if over else 1.0) and wgt[i] == w1[0]
            Hs += w1[0] * (J[0].T @ J[0])
            gs += w1[0] * (J[0].T @ r[0])
        assert np.abs(H - Hs).max() <= 1e-12 * np.abs(Hs).max() and np.abs(g - gs).max() <= 1e-12 * max(1.0, np.abs(gs).max())
        h = 1e-6
        num = np.zeros(6)
        for a in range(6):
            d = np.zeros(6)
            d[a] = h
            num[a] = (rho_sum(pb, f, SR.update(P[f], d)) - rho_sum(pb, f, SR.update(P[f], -d))) / (2 * h)
        assert np.abs(num - 2 * g).max() <= 1e-5 * max(1.0, np.abs(g).max()), (name, f, num, 2 * g)


def test_loss_values():
    """the three branches of the loss on hand-made residuals"""
    cam = (100.0, 100.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    Xw = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    uv = np.array([[0.3, 0.4], [3.0, 4.0], [0.6, 0.8], [0.0, 0.0]])       # |r| = 0.5, 5, 1 (at the threshold), behind
    rho, wgt, over, ok = SR.corner_terms(LR.OneCamera(cam), np.eye(3), np.zeros(3), Xw, uv, np.zeros(4, dtype=np.int64), 1.0)
    assert ok.tolist() == [True, True, True, False] and over.tolist() == [False, True, False, False]
    assert abs(rho[0] - 0.25) <= 1e-15 and abs(rho[1] - 9.0) <= 1e-14 and abs(rho[2] - 1.0) <= 1e-15 and rho[3] == 1e12
    assert wgt[0] == 1.0 and abs(wgt[1] - 0.2) <= 1e-16 and wgt[2] == 1.0 and wgt[3] == 0.0


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_shapes_exercise_both_branches(name):
    """in every linearisation of a shape case (the chain's and the three trials') at least one corner is over and one under
    the threshold: the device comparison runs both branches of the loss; status 0, all trials run"""
    out, res, trace = RC.statement(name)
    pb = trace["problem"]
    assert res["status"] == 0 and res["iterations"] == SC.COMPARE_ITERS and len(trace["lins"]) == SC.COMPARE_ITERS + 1
    for P, lin in trace["lins"]:
        over = under = 0
        for f in range(pb.n):
            if pb.pts[f] is not None:
                wgt = pb.frame(f, P[f])[4]
                over += int((wgt < 1).sum())
                under += int((wgt == 1).sum())
        assert over >= 1 and under >= 1, (name, over, under)
    assert res["n_soft"] == out["n_rejected"].sum() >= 1 and out["n_rejected"][0] >= 1


def test_scene_soft_counts_are_not_decided_by_rounding():
    out, res, trace = RC.statement("scene")
    pb, P = trace["problem"], trace["P"]
    margin = min(float(np.nanmin(np.abs(pb.frame(f, P[f])[5] - RC.SCENE_HUBER))) for f in range(pb.n))
    print("least | |r| - k | at the scene's returned poses: %.3g px" % margin)
    assert margin > 1e-6


def test_recorded_figures_still_hold():
    r = RC.recorded()
    obs, rec, seed, truth = RC.scene()
    out, res, _ = RC.statement("scene")
    plain, pres, _ = SC.run(obs, rec, seed, None, SC.NOISE_SIGMAS, max_iters=RC.SCENE_ITERS)
    seeds, robust, squared = RC.rmse(seed["T"], truth), RC.rmse(out["T"], truth), RC.rmse(plain["T"], truth)
    print("scene: seeds %.6g, plain %.6g (%d trials), robust %.6g (%d trials, n_soft %d, frames %s)" %
          (seeds, squared, pres["iterations"], robust, res["iterations"], res["n_soft"], np.flatnonzero(out["n_rejected"]).tolist()))
    assert res["status"] == 0 and pres["status"] == 0
    assert 0.99 * r["scene_rmse_seed"] <= seeds <= r["scene_rmse_seed"]
    assert r["scene_rmse_plain"] <= squared <= 1.01 * r["scene_rmse_plain"]
    assert 0.99 * r["scene_rmse_robust"] <= robust <= r["scene_rmse_robust"] and RC.up4(robust) == r["scene_rmse_robust"]
    assert robust <= 0.1 * squared                  # the condition; the figures say a hundredth and better
    assert res["iterations"] == r["scene_trials"] and res["n_soft"] == r["scene_soft"] == out["n_rejected"].sum()
    assert (out["n_rejected"][RC.SCENE_FRAMES] > 0).all()
    co, cr, cs, ct = RC.scene(False)
    clean, cres, _ = RC.run(co, cr, cs, None, SC.NOISE_SIGMAS, RC.SCENE_HUBER, RC.SCENE_ITERS)
    cp = SC.statement("noise")[0]
    a, b = RC.rmse(clean["T"], ct), RC.rmse(cp["T"], ct)
    print("clean: robust %.7g (%d trials, n_soft %d), plain %.7g" % (a, cres["iterations"], cres["n_soft"], b))
    assert abs(a - b) <= 0.01 * b and a <= r["clean_rmse_robust"] and b <= SC.recorded()["noise_rmse_smooth"]


def test_robust_tolerance():
    """ROBUST_TOL's rule, measured again: the statement against itself with reversed corner sums over every case and batch"""
    worst, at = 0.0, None
    runs = [(c[0],) + c[1:] for c in RC.all_cases()]
    for which, b in (("ragged", RC.ragged()), ("mixed", RC.mixed())):
        for k, (a0, a1) in enumerate(SQ.ranges(b)):
            runs.append(("%s[%d]" % (which, k), b.obs[a0:a1], b.rec, b.seed[a0:a1], b.dist, b.sigmas, b.huber, b.max_iters))
    for name, obs, rec, seed, dist, sig, huber, iters in runs:
        a, ra, _ = RC.run(obs, rec, seed, dist, sig, huber, iters)
        b, rb, _ = RC.run(obs, rec, seed, dist, sig, huber, iters, reverse=True)
        assert ra["status"] == rb["status"] and ra["iterations"] == rb["iterations"] and np.array_equal(a["n_rejected"], b["n_rejected"]), name
        if not np.all(np.isfinite(a["T"])):
            continue
        e = max(LC.rel_err(x, y) for x, y in zip(a["T"], b["T"]))
        if e > worst:
            worst, at = e, name
    print("largest rel_err under reversed sums: %.4g at %s" % (worst, at))
    assert worst <= RC.ROBUST_TOL_MEASURED and RC.ROBUST_TOL == max(10 * RC.ROBUST_TOL_MEASURED, 1e-9)
    assert [int(RC.batch_statement("mixed", k)[1]["status"]) for k in range(4)] == RC.MIXED_STATUS


@pytest.mark.parametrize("name", ["shape5_4_0", "shape65_4_0", "shape5_20_5", "scene"])
def test_covariance_is_the_dense_inverse_of_the_weighted_matrix(name):
    _, obs, rec, seed, dist, sig, huber, iters = [c for c in RC.all_cases() if c[0] == name][0]
    out, res, _ = RC.statement(name)
    cov = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig, huber)[0]
    pb = SV.problem_blocks(obs, rec, SC.K, dist, SC.TAG, out, *sig, huber)[0]
    assert (cov["status"] == 0).all() and (cov["dof"] == 8 * int(pb.n_tags.sum()) - 6).all() and (cov["sigma_px"] == sig[0]).all()
    dense, A = SV.dense_marginals(obs, rec, SC.K, dist, SC.TAG, out, *sig, huber)
    for f in range(len(out)):
        CK.assert_cov_close(cov["cov"][f], dense[f], A, (name, f))
    # a down-weighted corner gives less information: no frame is tighter than under the squared loss at the same poses
    plain = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig)[0]
    soft = np.flatnonzero(out["n_rejected"])
    assert len(soft) and (SV.position_std(cov["cov"])[soft] > SV.position_std(plain["cov"])[soft]).all()
