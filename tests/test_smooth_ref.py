"""The sequence localisation without a GPU: the library's exports and record sizes, and the properties of the NumPy
statement tests/smooth_ref.py, with the figures tests/smooth_cases.py records measured again."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import smooth_cases as SC
import smooth_ref as SR
from aprilslam_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "aprilslam.h"


def test_library_exports_and_record_sizes():
    L = _lib.load()
    for name in ("asl_smooth_frames_device", "asl_smooth_batch"):
        assert name in _lib.EXPORTS
        assert C.cast(getattr(L, name), C.c_void_p).value
    text = HEADER.read_text()
    stated = int(re.search(r"\}\s*asl_smooth_result;\s*/\*\s*(\d+) bytes", text).group(1))
    assert _lib.SMOOTH_RESULT_DTYPE.itemsize == stated == 64
    assert int(re.search(r"\}\s*asl_cam_pose;\s*/\*\s*(\d+) bytes", text).group(1)) == _lib.CAM_POSE_DTYPE.itemsize
    # NULL detector: refused before anything is touched (a host path: no GPU needed)
    assert L.asl_smooth_batch(None, None, 1, 1, None, 1, None, None, 0, 1.0, None, 1.0, 1.0, 1.0, 1, None, None) == -1


def random_pose(rng, angle, shift):
    w = rng.normal(size=3)
    return LR.rodrigues(w / np.linalg.norm(w) * angle), rng.normal(size=3) * shift


@pytest.mark.parametrize("angle,tol", [(1e-3, 1e-3), (0.0, 1e-6)])
def test_motion_jacobians_against_central_differences(angle, tol):
    rng = np.random.default_rng(3)
    sr, st, h = 0.02, 0.3, 1e-6
    for _ in range(5):
        Pa = random_pose(rng, 0.7, 2.0)
        dR, dt = random_pose(rng, angle, 0.4)
        Pb = (dR @ Pa[0], dR @ Pa[1] + dt)
        Jn, Jp = SR.motion_jacobians(*SR.relative(Pa, Pb), 1.0 / sr, 1.0 / st)
        num_n, num_p = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            num_n[:, k] = (SR.motion_residual(Pa, SR.update(Pb, e), sr, st) - SR.motion_residual(Pa, SR.update(Pb, -e), sr, st)) / (2 * h)
            num_p[:, k] = (SR.motion_residual(SR.update(Pa, e), Pb, sr, st) - SR.motion_residual(SR.update(Pa, -e), Pb, sr, st)) / (2 * h)
        for J, num in ((Jn, num_n), (Jp, num_p)):
            err = np.abs(J - num).max() / np.abs(num).max()
            print("relative rotation %g: Jacobian error %.3g" % (angle, err))
            assert err <= tol


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_block_tridiagonal_solve_against_the_dense_one(n):
    rng = np.random.default_rng(10 + n)
    J = rng.normal(size=(12 * n, 6 * n))
    A = J.T @ J
    for f in range(n):      # keep the tridiagonal part
        for g in range(n):
            if abs(f - g) > 1:
                A[6 * f:6 * f + 6, 6 * g:6 * g + 6] = 0
    A += 6 * n * np.eye(6 * n)      # diagonally dominant: positive definite after the cut
    D = np.array([A[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(n)])
    Cc = np.array([A[6 * f + 6:6 * f + 12, 6 * f:6 * f + 6] for f in range(n - 1)]).reshape(n - 1, 6, 6)
    b = rng.normal(size=(n, 6))
    assert np.array_equal(SR.dense(D, Cc), A)
    for lam in (0.0, 1e-3, 10.0):
        x = SR.tridiag_solve(D, Cc, b, lam)
        want = np.linalg.solve(A + lam * np.diag(np.diag(A)), b.reshape(-1))
        assert np.abs(x.reshape(-1) - want).max() <= 1e-10 * np.abs(want).max()
    D[n // 2] = -D[n // 2]
    assert SR.tridiag_solve(D, Cc, b, 1e-3) is None


def test_one_frame_is_the_localisation_refinement():
    obs, rec, seed, _ = SC.noise()
    out, res, _ = SR.smooth(obs[:1], rec, SC.K, None, SC.TAG, seed[:1], 1.0, 0.01, 0.1, LR.LM_ITERS)
    model = LR.OneCamera(LR.camera(SC.K, None))
    part = LR.gather(obs[0], rec)[1]
    Xw, uv, ci = LR.frame_points(model, obs[0], rec, SC.TAG, part)
    R, t, cost = LR.lm(LR.model_lin(model, Xw, uv, ci), *SR.pose_of_seed(seed[0]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
    assert res["status"] == 0 and out["status"][0] == 0 and LC.rel_err(out["T"][0], T) <= 1e-13
    assert abs(res["cost"] - cost) <= 1e-12 * cost and abs(out["rms_px"][0] - np.sqrt(cost / (4 * len(part)))) <= 1e-12


def test_a_prior_of_no_weight_leaves_the_localisation():
    obs, rec, seed, _ = SC.noise()
    out, res, _ = SR.smooth(obs[:12], rec, SC.K, None, SC.TAG, seed[:12], 1.0, 1e6, 1e6, SC.MAX_ITERS)
    assert res["status"] == 0 and (out["status"] == 0).all()
    worst = max(LC.rel_err(o, s) for o, s in zip(out["T"], seed["T"][:12]))
    print("largest distance from the per-frame localisation %.3g" % worst)
    assert worst <= 1e-7


def test_holes():
    obs, rec, seed, truth = SC.holes()
    out, res, _ = SC.statement("holes")
    assert res["status"] == 0 and res["n_filled"] == 3 and res["n_frames_data"] == 4 and res["n_flipped"] == 0
    assert out["status"].tolist() == [6, 0, 0, 6, 0, 0, 6] and out["seed_slot"][[0, 3, 6]].tolist() == [-1, -1, -1]
    p = out["T"][:, :3, 3]
    along = (p[3] - p[2]) @ (p[4] - p[2]) / ((p[4] - p[2]) @ (p[4] - p[2]))
    assert 0.4 <= along <= 0.6
    err = SC.pos_err(out["T"], truth)
    rec_ = SC.recorded()
    print("position error of the filled frames", err[[0, 3, 6]])
    for got, key in ((max(err[0], err[6]), "holes_end_err"), (err[3], "holes_mid_err")):
        assert 0.9 * rec_[key] <= got <= rec_[key], (key, got)


@pytest.mark.parametrize("first", [False, True])
def test_flips(first):
    obs, rec, seed, truth, frames = SC.flips(first)
    out, res, trace = SC.statement("flips_first" if first else "flips")
    assert res["status"] == 0 and (out["status"] == 0).all()
    assert np.flatnonzero(trace["choice"]).tolist() == list(frames) and res["n_flipped"] == len(frames)
    assert np.flatnonzero(out["seed_slot"] == seed["seed_slot"] + SR.FLIPPED).tolist() == list(frames)
    final, seeds = SC.flip_errors(out["T"], first)
    key = "flips_first_margin" if first else "flips_margin"
    print("final %.4g rad, seeds %.4g rad, ratio %.4g" % (final, seeds, final / seeds))
    assert 0.9 * SC.recorded()[key] <= final / seeds <= SC.recorded()[key]
    # the mirrored seeds themselves are far off: the chain, not the LM, brings them back
    assert min(LC.rot_err(seed["T"][f], truth[f]) for f in frames) > 20 * final


def test_noise_is_averaged():
    obs, rec, seed, truth = SC.noise()
    out, res, _ = SC.statement("noise")
    assert res["status"] == 0 and (out["status"] == 0).all()
    frame = float(np.sqrt(np.mean(SC.pos_err(seed["T"], truth) ** 2)))
    smooth = float(np.sqrt(np.mean(SC.pos_err(out["T"], truth) ** 2)))
    print("position RMSE per frame %.4g, smoothed %.4g, sigmas %s" % (frame, smooth, SC.NOISE_SIGMAS))
    r = SC.recorded()
    assert 0.99 * r["noise_rmse_frame"] <= frame <= r["noise_rmse_frame"]
    assert 0.99 * r["noise_rmse_smooth"] <= smooth <= r["noise_rmse_smooth"]
    assert smooth <= 0.5 * frame
    assert res["rms_px"] >= res["rms_seed_px"] and res["cost"] < res["cost_seed"]   # the prior costs the corners a little


def test_device_tolerance_and_chain_margins():
    """the statement against itself with reversed corner sums, every case; and no case has a near-tie in its chain"""
    worst = 0.0
    for name, obs, rec, seed, dist, sig, iters in SC.all_cases():
        a, ra, trace = SC.statement(name)
        b, rb, _ = SC.run(obs, rec, seed, dist, sig, reverse=True, max_iters=iters)
        e = max(LC.rel_err(x, y) for x, y in zip(a["T"], b["T"]))
        print("%-14s rel_err %.3g trials %d / %d chain margin %.3g" % (name, e, ra["iterations"], rb["iterations"], SC.chain_margin(trace)))
        worst = max(worst, e)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["seed_slot"], b["seed_slot"])
        assert ra["iterations"] == rb["iterations"], name      # no case sits in the rounding-decided tail
        if iters == SC.COMPARE_ITERS and ra["status"] == 0:
            assert ra["iterations"] == iters, name              # the comparison cases run all their trials
        assert SC.chain_margin(trace) >= 1e-3, name
    print("worst %.4g" % worst)
    assert worst <= SC.DEVICE_TOL_MEASURED
    assert SC.DEVICE_TOL == max(10 * SC.DEVICE_TOL_MEASURED, 1e-9)


def test_edge_sequences_of_the_statement():
    out, res, _ = SC.statement("all_empty")
    assert res["status"] == 1 and (out["status"] == 1).all() and all(np.array_equal(T, np.eye(4)) for T in out["T"])
    for name, posed in (("first_only", 0), ("last_only", 5)):
        out, res, _ = SC.statement(name)
        assert res["status"] == 0 and res["n_filled"] == 5
        assert [s for f, s in enumerate(out["status"]) if f != posed] == [6] * 5 and out["status"][posed] == 0
        for T in out["T"]:      # a random walk from one pose stays there
            assert LC.rel_err(T, out["T"][posed]) <= 1e-9
    out, res, _ = SC.statement("hole70")
    assert res["status"] == 0 and res["n_filled"] == 70 and (out["status"][2:72] == 6).all()


@pytest.mark.parametrize("name", ["behind", "nonfinite"])
def test_solves_that_fail(name):
    obs, rec, seed, sig, iters, status, trials = SC.failure_cases()[name]
    out, res, _ = SC.run(obs, rec, seed, None, sig, max_iters=iters)
    assert res["status"] == status and res["iterations"] == trials and (out["status"] == SR.FRAME_FAILED).all()
    assert (out["n_tags"] == 4).all() and res["n_frames_data"] == len(obs)
    if name == "behind":    # the chain's pose comes back, and every corner costs 1e12
        assert LC.rel_err(out["T"][0], seed["T"][0]) <= 1e-15 and res["cost"] == res["cost_seed"] == 16 * 1e12 / sig[0] ** 2
    else:
        assert not np.isfinite(res["cost_seed"])
