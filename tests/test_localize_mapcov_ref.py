"""Monte Carlo of the propagation tests/localize_mapcov_ref.py states: a camera localised against a map whose tags are off by a
draw from a joint covariance Sigma_map, from corners with Gaussian noise.  The pose errors must have the covariance the
statement predicts from Sigma_map and the corner sigma -- and not the pixel-only sigma^2 (J^T J)^-1, which is what a map
taken as exact gives.

The experiment: the bench scene (20 tags in view), the camera at trajectory(16)[2]; the world tag, the lowest id in view,
exact; every other tag off by 2 mrad and 0.05 units of its own plus 1 mrad and 0.03 units common to all
(localize_mapcov_cases.synthetic_cov); corner noise 0.3 px; N = 400 samples, fixed seed.  Bars, from the sampling
distributions alone: the mean Mahalanobis^2 of a chi^2_6 (variance 12) over N samples within 4 sqrt(12 / N) of 6; every
component's empirical / predicted std within 1 +- 4 / sqrt(2 N) (the relative std of a sample std is 1 / sqrt(2 N))."""
import numpy as np
import pytest

import localize_cases as LC
import localize_mapcov_cases as LMC
import localize_mapcov_ref as LMR
import localize_ref as LR
import pose_cov_ref as PC
from aprilslam_amd import synth
from aprilslam_amd.localize import TagMap

N, SIGMA, SEED = 400, 0.3, 7


@pytest.fixture(scope="module")
def experiment():
    K = synth.camera_matrix(LC.W, LC.H)
    tags = LC.bench_scene()
    true_map = TagMap.from_scene(tags).as_records()
    pos, rot = LC.trajectory(16)[2]
    row = LC.exact_frame(tags, pos, rot, K)
    seen = [int(i) for i in row["id"] if i >= 0]
    assert len(seen) == 20
    ids = sorted(seen)[1:]                                  # the world tag, the lowest id in view, is exact
    Sigma = LMC.synthetic_cov(ids)
    slot = LMC.cov_slot(ids, len(true_map))
    model = LR.OneCamera(LR.camera(K, None))
    T_true = LC.world_from_camera(pos, rot)
    R, t = T_true[:3, :3].T, -T_true[:3, :3].T @ T_true[:3, 3]
    active = list(range(len(seen)))
    Xw, uv, ci = LR.frame_points(model, row, true_map, LC.TAG_INNER, active)
    pred, _, dof, status = LMR.pose_cov(model, R, t, Xw, uv, ci, seen, SIGMA, slot, Sigma)
    pixel, _, _, _ = LR.pose_cov(model, R, t, Xw, uv, ci, SIGMA)
    marg = np.zeros_like(Sigma)                             # the per-tag marginals alone: what a tag std could carry
    for k in range(len(ids)):
        marg[6 * k:6 * k + 6, 6 * k:6 * k + 6] = Sigma[6 * k:6 * k + 6, 6 * k:6 * k + 6]
    pred_marg = LMR.pose_cov(model, R, t, Xw, uv, ci, seen, SIGMA, slot, marg)[0]
    assert status == 0 and dof == 8 * 20 - 6
    rng = np.random.default_rng(SEED)
    Lc = np.linalg.cholesky(Sigma)
    errs = []
    for _ in range(N):
        est_map = LMC.perturbed(true_map, ids, Lc @ rng.normal(size=len(Sigma)))
        noisy = row.copy()
        noisy["corners"] += rng.normal(0, SIGMA, noisy["corners"].shape).astype(np.float32)
        out, Rt, act, _ = LR.solve_frame(model, noisy, est_map, LC.TAG_INNER, 0.0)
        assert out["status"] == 0 and len(act) == 20
        errs.append(PC.pose_error(out["T"][:3, :3], out["T"][:3, 3], T_true[:3, :3], T_true[:3, 3]))
    return np.array(errs), pred, pixel, pred_marg


def test_mahalanobis_mean(experiment):
    errs, pred, _, _ = experiment
    m2 = np.einsum('ni,ij,nj->n', errs, np.linalg.inv(pred), errs)
    print("mean Mahalanobis^2", m2.mean(), "+-", m2.std() / np.sqrt(N))
    assert abs(m2.mean() - 6) <= 4 * np.sqrt(12 / N), m2.mean()


def test_every_component(experiment):
    errs, pred, _, _ = experiment
    ratio = errs.std(axis=0) / np.sqrt(np.diag(pred))
    print("empirical / predicted std", ratio)
    assert np.abs(ratio - 1).max() <= 4 / np.sqrt(2 * N), ratio


def test_pixel_only_prediction_is_far_off(experiment):
    """what keeps the test meaningful: a map taken as exact under-states every component more than five times"""
    errs, _, pixel, _ = experiment
    ratio = errs.std(axis=0) / np.sqrt(np.diag(pixel))
    print("empirical / pixel-only std", ratio)
    assert ratio.min() > 5, ratio


def test_marginals_alone_differ(experiment):
    """the blocks between tags matter: the prediction from the per-tag marginals alone differs from the joint one by more
    than the Monte Carlo bar on some component"""
    _, pred, _, pred_marg = experiment
    ratio = np.sqrt(np.diag(pred_marg) / np.diag(pred))
    print("marginals-only / joint predicted std", ratio)
    assert np.abs(ratio - 1).max() > 4 / np.sqrt(2 * N), ratio


def test_exact_tags_and_statuses():
    K = synth.camera_matrix(LC.W, LC.H)
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    pos, rot = LC.trajectory(16)[2]
    row = LC.exact_frame(tags, pos, rot, K)
    model = LR.OneCamera(LR.camera(K, None))
    out, Rt, act, _ = LR.solve_frame(model, row, rec, LC.TAG_INNER, 0.0)
    ids = sorted(int(i) for i in row["id"] if i >= 0)[1:]
    Sigma = LMC.synthetic_cov(ids)
    none = np.full(len(rec), -1, dtype=np.int32)
    plain = LR.frame_cov(model, row, rec, LC.TAG_INNER, Rt, act, SIGMA)
    got = LMR.frame_cov(model, row, rec, LC.TAG_INNER, Rt, act, SIGMA, none, Sigma)
    assert got.tobytes() == plain.tobytes()                 # every slot -1: the pixel-only record
    slot = LMC.cov_slot(ids, len(rec))
    full = LMR.frame_cov(model, row, rec, LC.TAG_INNER, Rt, act, SIGMA, slot, Sigma)
    assert full["status"] == 0 and np.array_equal(full["cov"], full["cov"].T)
    assert np.linalg.eigvalsh(full["cov"] - plain["cov"]).min() > 0      # the map only adds
    bad = slot.copy()
    bad[ids[3]] = len(ids)
    assert LMR.frame_cov(model, row, rec, LC.TAG_INNER, Rt, act, SIGMA, bad, Sigma)["status"] == LMR.STATUS_BAD_MAP_COV
    nan = Sigma.copy()
    nan[7, 20] = np.nan
    r3 = LMR.frame_cov(model, row, rec, LC.TAG_INNER, Rt, act, SIGMA, slot, nan)
    assert r3["status"] == LMR.STATUS_BAD_MAP_COV and not r3["cov"].any()
    assert LMR.frame_cov(model, row, rec, LC.TAG_INNER, None, [], SIGMA, slot, Sigma)["status"] == PC.STATUS_NO_POSE
