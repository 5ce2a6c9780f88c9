"""The NumPy statement of the smoothed poses' covariance (tests/smooth_cov_ref.py) against an independent second route, the
per-frame localisation's covariance, the statistics of sequences drawn from its own prior, and the recorded figures of
tests/smooth_cov_cases.py.  No GPU."""
import numpy as np
import pytest

import localize_ref as LR
import pose_cov_ref as PC
import smooth_cases as SC
import smooth_cov_cases as VC
import smooth_cov_ref as SV
import smooth_ref as SR
import solver_checks as CK

ALL = [c[0] for c in SC.all_cases()]


@pytest.mark.parametrize("name", ALL)
def test_recursion_matches_the_dense_inverse(name):
    obs, rec, seed, dist, sig, iters = VC.case(name)
    poses, res = VC.statement(name)
    cov = VC.statement_cov(name)
    assert np.array_equal(cov["sigma_px"], np.full(len(poses), sig[0]))
    if name == "all_empty":
        assert (cov["status"] == 1).all()
        return
    pb, P, D, C = SV.problem_blocks(obs, rec, SC.K, dist, SC.TAG, poses, *sig)
    ratio = SV.min_pivot_ratio(D, C)
    assert ratio >= VC.recorded()["pivot_floor"], (name, ratio)
    assert (cov["status"] == 0).all() and (cov["dof"] == 8 * int(pb.n_tags.sum()) - 6).all()
    dense, A = SV.dense_marginals(obs, rec, SC.K, dist, SC.TAG, poses, *sig)
    for f in range(len(poses)):
        CK.assert_cov_close(cov["cov"][f], dense[f], A, (name, f))


@pytest.mark.parametrize("name", ["shape1_1_0", "shape1_4_0"])
def test_one_frame_is_the_localisation_covariance(name):
    obs, rec, seed, dist, sig, iters = VC.case(name)
    poses, res = VC.statement(name)
    cov = VC.statement_cov(name)
    pb = SR.problem(obs, rec, SC.K, dist, SC.TAG, *sig)
    R, t = SR.pose_of_seed(poses[0])
    Xw, uv, ci = LR.frame_points(pb.model, obs[0], rec, SC.TAG, pb.part[0])
    want, sigma, dof, status = LR.pose_cov(pb.model, R, t, Xw, uv, ci, sig[0])
    assert status == 0 and cov["status"][0] == 0 and cov["dof"][0] == dof and cov["sigma_px"][0] == sigma
    H = pb.model.linearise(R, t, Xw, uv, ci)[1]
    CK.assert_cov_close(cov["cov"][0], want, H, name)


def test_nees_of_sequences_drawn_from_the_prior():
    """what makes the definition a covariance: over runs whose motion is drawn from the prior and whose corners carry the
    assumed noise, a frame's mean e^T C^-1 e is 6 with standard deviation sqrt(12 / runs)"""
    nees = np.array([VC.nees_of_run(r) for r in range(VC.NEES_RUNS)])
    mean = nees.mean(axis=0)
    print("mean NEES per frame", np.array2string(mean, precision=3), "overall %.3f, band 6 +- %.3f" % (nees.mean(), VC.NEES_BAND))
    assert np.all(np.abs(mean - 6.0) <= VC.NEES_BAND), mean


def test_holes_structure():
    std = SV.position_std(VC.statement_cov("holes")["cov"])
    print("holes position std", np.array2string(std, precision=5))
    rec = VC.recorded()
    assert abs(std[0] - rec["holes_end_std"]) <= VC.DIGITS and abs(std[6] - rec["holes_end_std"]) <= VC.DIGITS
    assert abs(std[3] - rec["holes_mid_std"]) <= VC.DIGITS
    data = std[[1, 2, 4, 5]]
    assert rec["holes_data_std"][0] <= data.min() and data.max() <= rec["holes_data_std"][1]
    assert min(std[0], std[6]) > std[3] > data.max()
    # the analytic values of a neighbour without uncertainty lie just below
    st = SC.HOLES_SIGMAS[2]
    assert 0 < rec["holes_end_std"] - np.sqrt(3) * st < 2e-3 and 0 < rec["holes_mid_std"] - np.sqrt(1.5) * st < 2e-3


def test_hole70_structure():
    std = SV.position_std(VC.statement_cov("hole70")["cov"])
    peak, value = VC.recorded()["hole70_peak"]
    rims = VC.recorded()["hole70_rims"]
    print("hole70 position std: frame 1 %.5f, frame %d %.5f, frame 72 %.5f" % (std[1], int(np.argmax(std)), std.max(), std[72]))
    assert int(np.argmax(std)) == peak and abs(std[peak] - value) <= VC.DIGITS
    assert abs(std[1] - rims[0]) <= VC.DIGITS and abs(std[72] - rims[1]) <= VC.DIGITS
    assert np.all(np.diff(std[1:peak + 1]) > 0) and np.all(np.diff(std[peak:73]) < 0)


@pytest.mark.parametrize("name", VC.NO_SOLVE_CASES)
def test_no_solve_no_covariance(name):
    sig = VC.case(name)[4]
    poses, res = VC.statement(name)
    cov = VC.statement_cov(name)
    assert res["status"] != 0 and np.all(np.isin(poses["status"], (1, 4)))
    assert (cov["status"] == 1).all() and not cov["cov"].any() and (cov["dof"] == 0).all() and (cov["sigma_px"] == sig[0]).all()


def test_prior_only_is_not_positive_definite():
    poses, res = VC.statement("prior_only")
    cov = VC.statement_cov("prior_only")
    assert res["status"] == 0 and (poses["status"] == 6).all()
    assert (cov["status"] == 2).all() and not cov["cov"].any() and (cov["dof"] == -6).all()
    assert (cov["sigma_px"] == SC.HOLES_SIGMAS[0]).all()
