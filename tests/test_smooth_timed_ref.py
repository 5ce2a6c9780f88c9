"""The NumPy statement of the sequence localisation (tests/smooth_ref.py) with frame times against the same statement without
them where the two must agree, and the figures recorded in tests/smooth_timed_cases.py measured again.  CPU only."""
import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_ref as SR
import smooth_seq_cases as SQ
import smooth_timed_cases as TC

PLAIN = {c[0]: c[1:] for c in SC.all_cases()}


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", list(PLAIN))
def test_unit_spacing_is_the_plain_statement(name):
    """times = c + f with exact differences, and no times at all: smooth_ref.smooth's bytes, with and without Huber"""
    obs, rec, seed, dist, sig, iters = PLAIN[name]
    for huber in (0.0, 0.6):
        want = SC.statement(name) if huber == 0.0 else SC.run(obs, rec, seed, dist, sig, max_iters=iters, huber=huber)
        for times in (None, 5.0 + np.arange(len(obs))):
            assert same(TC.run(obs, rec, seed, dist, times, sig, max_iters=iters, huber=huber), want), (name, huber, times)


def test_times_change_the_answer():
    """the irregular times are not a no-op: every case with a pair moves, and the weights are the stated ones"""
    for name in ("shape2_4_0", "shape65_4_0", "hole70"):
        obs, rec, seed, dist, times, sig, iters = TC.case(name)
        assert not same(TC.statement(name), SC.statement(name)), name
    obs, rec, seed, dist, times, sig, iters = TC.case("shape1_4_0")
    assert same(TC.statement("shape1_4_0"), SC.statement("shape1_4_0"))       # one frame: no pair, no transition
    pb = TC.statement("shape5_4_0")[2]["problem"]
    for f in range(4):
        dt = pb.times[f + 1] - pb.times[f]
        assert pb.pair_weights(f) == ((1.0 / sig[1]) * (1.0 / np.sqrt(dt)), (1.0 / sig[2]) * (1.0 / np.sqrt(dt)))
    # the chain of hole70 divides by the time across the hole
    tr_timed, tr_plain = TC.statement("hole70")[2]["tr"], SC.statement("hole70")[2]["tr"]
    t = TC.case("hole70")[4]
    posed = TC.statement("hole70")[2]["posed"]
    k = posed.index(72)
    assert posed[k - 1] == 1 and np.allclose(tr_timed[k] * (t[72] - t[1]), tr_plain[k] * 71.0, rtol=1e-14)


def test_a_scaled_clock_is_a_scaled_sigma():
    """times in another unit with the sigmas per that unit: the same problem (to rounding: sqrt(4 dt) = 2 sqrt(dt) exactly)"""
    obs, rec, seed, dist, times, sig, iters = TC.case("shape5_4_0")
    a = TC.statement("shape5_4_0")
    b = TC.run(obs, rec, seed, dist, 4.0 * times, (sig[0], sig[1] / 2.0, sig[2] / 2.0), max_iters=iters)
    assert TC.worst_rel(a[0]["T"], b[0]["T"]) <= 1e-12 and abs(a[1]["cost"] - b[1]["cost"]) <= 1e-12 * a[1]["cost"]


def test_device_tolerance_and_chain_margins():
    """the statement against itself with reversed corner sums, every timed case; no case has a near-tie in its chain"""
    worst = 0.0
    for name, obs, rec, seed, dist, times, sig, iters in TC.all_cases():
        a, ra, trace = TC.statement(name)
        b, rb, _ = TC.run(obs, rec, seed, dist, times, sig, reverse=True, max_iters=iters)
        e = TC.worst_rel(a["T"], b["T"])
        print("%-14s rel_err %.3g trials %d / %d chain margin %.3g" % (name, e, ra["iterations"], rb["iterations"], SC.chain_margin(trace)))
        worst = max(worst, e)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["seed_slot"], b["seed_slot"])
        assert ra["iterations"] == rb["iterations"], name
        if ra["status"] == 0:
            assert ra["iterations"] == SC.COMPARE_ITERS, name
        assert SC.chain_margin(trace) >= 1e-3, name
    print("worst %.4g" % worst)
    assert worst <= TC.DEVICE_TOL_MEASURED
    assert TC.DEVICE_TOL == max(10 * TC.DEVICE_TOL_MEASURED, 1e-9)


def test_dropped_frames_are_marginalised():
    """timed on the kept frames of the gap scene = the plain statement on all frames with the gap emptied, at the kept frames"""
    timed, naive, emptied = TC.gap_statements()
    k = TC.kept_frames()
    assert timed[1]["status"] == 0 and emptied[1]["status"] == 0 and emptied[1]["n_filled"] == TC.GAP[1] - TC.GAP[0]
    e = TC.worst_rel(timed[0]["T"], emptied[0]["T"][k])
    print("gap scene: timed against emptied %.4g (recorded %.4g), trials %d / %d" % (e, TC.recorded()["marg_gap"], timed[1]["iterations"],
                                                                                    emptied[1]["iterations"]))
    assert e <= 10 * TC.recorded()["marg_gap"]
    assert abs(timed[1]["cost"] - emptied[1]["cost"]) <= 1e-9 * emptied[1]["cost"]       # the same minimum
    assert TC.worst_rel(naive[0]["T"], emptied[0]["T"][k]) > 1e-3                        # which the naive call does not find


def test_a_half_step_grid_is_the_doubled_grid():
    (obs, rec, seed, times), (wide, _, wseed, g) = TC.half_grid()
    assert np.array_equal(times * 2, np.round(times * 2)) and set(np.diff(times)) == {0.5, 1.0, 1.5}
    s = TC.GAP_SIGMAS
    timed = TC.run(obs, rec, seed, None, times, s)
    r = np.sqrt(0.5)
    plain = SC.run(wide, rec, wseed, None, (s[0], s[1] * r, s[2] * r))
    assert timed[1]["status"] == 0 and plain[1]["status"] == 0 and plain[1]["n_filled"] == len(wide) - len(obs)
    e = TC.worst_rel(timed[0]["T"], plain[0]["T"][g])
    print("half-step grid: timed against the doubled grid %.4g (recorded %.4g)" % (e, TC.recorded()["marg_half"]))
    assert e <= 10 * TC.recorded()["marg_half"]


def test_pose_at():
    timed, _, emptied = TC.gap_statements()
    _, _, _, truth = TC.gap_scene()
    k = TC.kept_frames()
    times = k.astype(np.float64)
    for i, f in enumerate(k):       # a frame's own time: that frame's pose
        assert LC.rel_err(SR.pose_at(timed[0]["T"], times, float(f)), timed[0]["T"][i]) <= 1e-12
    rel = pos = truth_err = 0.0
    for f in range(*TC.GAP):        # the dropped frames' times: on the emptied-frames solve, to first order
        T = SR.pose_at(timed[0]["T"], times, float(f))
        rel = max(rel, LC.rel_err(T, emptied[0]["T"][f]))
        pos = max(pos, float(np.linalg.norm(T[:3, 3] - emptied[0]["T"][f][:3, 3])))
        truth_err = max(truth_err, float(np.linalg.norm(T[:3, 3] - truth[f][:3, 3])))
    r = TC.recorded()
    print("pose_at the dropped frames: rel_err %.4g (recorded %.4g), position %.4g (recorded %.4g), to the truth %.4g" %
          (rel, r["pose_at_rel"], pos, r["pose_at_pos"], truth_err))
    assert rel <= 2 * r["pose_at_rel"] and pos <= 2 * r["pose_at_pos"] and pos <= 0.05 * truth_err
    assert 0.9 * r["pose_at_rel"] <= rel <= r["pose_at_rel"] and 0.9 * r["pose_at_pos"] <= pos <= r["pose_at_pos"]
    # between two neighbouring frames it stays between them; no extrapolation; without times the index is the time
    mid = SR.pose_at(timed[0]["T"], times, 3.5)
    assert np.linalg.norm(mid[:3, 3] - 0.5 * (timed[0]["T"][3][:3, 3] + timed[0]["T"][4][:3, 3])) <= 1e-3
    assert np.allclose(mid[:3, :3] @ mid[:3, :3].T, np.eye(3), atol=1e-14)
    for t in (-0.5, 39.5, np.nan):
        with pytest.raises(ValueError):
            SR.pose_at(timed[0]["T"], times, t)
    assert np.array_equal(SR.pose_at(timed[0]["T"], None, 19.0), timed[0]["T"][19])
    with pytest.raises(ValueError):
        SR.pose_at(timed[0]["T"], None, 19.5)


def test_covariance_of_the_kept_frames():
    """the timed matrix's marginals at the kept frames = the emptied-frames matrix's (each at its own solve's poses)"""
    obs, rec, _, _ = TC.gap_scene()
    timed, _, emptied = TC.gap_statements()
    k = TC.kept_frames()
    s = TC.GAP_SIGMAS
    ct, A = SV.smooth_cov(obs[k], rec, SC.K, None, SC.TAG, timed[0], timed[1], *s, times=k.astype(np.float64))
    ce = SV.smooth_cov(TC.emptied_gap()[0], rec, SC.K, None, SC.TAG, emptied[0], emptied[1], *s)[0]
    assert (ct["status"] == 0).all() and (ce["status"] == 0).all() and A.shape == (120, 120)
    assert ct["dof"][0] == ce["dof"][0] == 8 * 4 * 20 - 6
    e = TC.scaled_cov_err(ct["cov"], ce["cov"][k])
    print("covariance at the kept frames: scaled error %.4g (recorded %.4g)" % (e, TC.recorded()["cov_scaled"]))
    assert e <= 2 * TC.recorded()["cov_scaled"]
    assert 0.9 * TC.recorded()["cov_scaled"] <= e <= TC.recorded()["cov_scaled"]
    # and against the independent route: the inverse of the assembled timed matrix
    Ai = np.linalg.inv(A)
    P = [SR.pose_of_seed(p) for p in timed[0]]
    import pose_cov_ref as PC
    for f in (0, 9, 10, 19):
        Am = PC.convention_map(P[f][0], P[f][1], True)
        want = Am @ Ai[6 * f:6 * f + 6, 6 * f:6 * f + 6] @ Am.T
        sd = np.sqrt(np.diag(want))
        assert (np.abs(ct["cov"][f] - want) / np.outer(sd, sd)).max() <= 1e-8
    # the naive matrix holds the gap as tightly as one frame step, so it is surer of the frames next to it (more information
    # on one link of the chain can only shrink a marginal)
    cn = SV.smooth_cov(obs[k], rec, SC.K, None, SC.TAG, timed[0], timed[1], *s)[0]
    assert (SV.position_std(cn["cov"])[[9, 10]] < SV.position_std(ct["cov"])[[9, 10]]).all()


def test_gap_scene_rmses():
    timed, naive, _ = TC.gap_statements()
    got, r = TC.gap_rmses(timed[0]["T"], naive[0]["T"]), TC.recorded()
    print("gap scene RMSE:", {k: "%.6g" % v for k, v in got.items()}, "naive / timed next to the gap %.3g" %
          (got["gap_naive_near"] / got["gap_timed_near"]))
    for key, v in got.items():
        assert 0.99 * r[key] <= v <= r[key], (key, v)
    assert got["gap_naive_near"] >= 1.5 * got["gap_timed_near"]
    assert got["gap_timed_all"] < got["gap_naive_all"] and got["gap_timed_near"] < got["gap_frame_near"]


def test_bad_times_are_status_4():
    b, times = TC.bad_times_batch()
    out, res = SR.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, b.seed, *b.sigmas, b.max_iters, times=times)
    assert res["status"].tolist() == TC.BAD_STATUS
    nothing = SC.statement("all_empty")
    for k, (a0, a1) in enumerate(SQ.ranges(b)):
        if TC.BAD_STATUS[k] == 0:
            alone = TC.run(b.obs[a0:a1], b.rec, b.seed[a0:a1], b.dist, times[a0:a1], b.sigmas, max_iters=b.max_iters)
            assert out[a0:a1].tobytes() == alone[0].tobytes() and res[k].tobytes() == alone[1].tobytes()
            assert out[a0:a1].tobytes() == TC.statement("shape5_4_0")[0].tobytes()
            continue
        assert SR.bad_times(times[a0:a1])
        want = nothing[1].copy()
        want["status"] = SR.BAD_TIMES
        assert res[k].tobytes() == want.tobytes()                                  # a status-1 result but for the status
        assert out[a0:a1].tobytes() == nothing[0][:a1 - a0].tobytes()               # status-1 frames: T identity, seed_slot -1
        cov, _ = SV.smooth_cov(b.obs[a0:a1], b.rec, SC.K, b.dist, SC.TAG, out[a0:a1], res[k], *b.sigmas, times=times[a0:a1])
        assert (cov["status"] == 1).all() and not cov["cov"].any() and (cov["dof"] == 0).all()
    # one frame needs only a finite time; infinities are not finite
    assert not SR.bad_times([3.0]) and SR.bad_times([np.inf]) and SR.bad_times([0.0, np.inf]) and not SR.bad_times([-2.0, -1.0])
    assert SR.bad_times([0.0, 0.0]) and SR.bad_times([1.0, 0.5]) and SR.bad_times([0.0, np.nan, 2.0])


def test_ragged_times_restart_at_every_boundary():
    b, times = TC.ragged()
    assert len(times) == len(b.obs) == 270
    for (a0, a1), (_, a2) in zip(SQ.ranges(b)[:-1], SQ.ranges(b)[1:]):
        assert (np.diff(times[a0:a1]) > 0).all() and (a1 - a0 == 1 or times[a1] < times[a1 - 1])
