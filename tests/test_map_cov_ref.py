"""The NumPy statement of the map's joint covariance (tests/map_cov_ref.py) against the statement of the map solve
(tests/map_ref.py): the dense inverse of the joint normal matrix at map_ref's own solution is symmetric, positive definite,
has no row for the world tag, and its diagonal is map_ref's tag_std -- which map_ref reads off a Cholesky factor, column by
column, as the device does.  So the matrix the device is compared with stands on the construction the std already rests on."""
import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_cov_ref as MCR
import map_ref as MR
import map_rig_cases as MRC
import map_robust_cases as MBC

K = MC.K_bench()
DIAG_RTOL = 1e-9


def check(ids, C, s2, res, tmap, std):
    """the properties of the statement matrix for a status-0 solve"""
    w = int(res["world_id"])
    assert res["status"] == 0
    assert ids == [int(i) for i in np.flatnonzero(tmap["valid"]) if i != w] and w not in ids      # no row for the world tag
    assert len(ids) == res["n_tags"] - 1 and C.shape == (6 * len(ids), 6 * len(ids))
    assert np.array_equal(C, C.T)
    assert s2 > 0 and np.isfinite(C).all()
    d = np.sqrt(np.diag(C))
    Cn = C / np.outer(d, d)                                                                        # the correlation matrix
    assert np.linalg.eigvalsh(Cn).min() > 0
    ref = np.concatenate([std[i] for i in ids])
    assert (ref > 0).all()
    err = np.abs(d / ref - 1).max()
    assert err <= DIAG_RTOL, err
    assert not np.any(std[w]) and all(not np.any(std[i]) for i in range(len(std)) if i not in ids)


@pytest.mark.parametrize("case", MC.cpu_cases(K), ids=lambda c: c[0])
def test_diagonal_is_the_tag_std(case):
    name, obs, dist, world = case
    res, tmap, std, poses, weight = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=world)
    ids, C, s2 = MCR.map_cov(obs, K, dist, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]))
    check(ids, C, s2, res, tmap, std)
    if name == "two_groups":            # no frame joins the groups: the second group is not mapped and has no block
        assert len(ids) < len({int(i) for i in obs["id"].ravel() if i >= 0}) - 1


def test_rig_with_several_views_of_a_pair():
    obs, rig = MRC.pair_block(6, 12, MRC.NOISE), MRC.PAIR
    views, pairs = MRC.view_counts(obs)
    assert views > pairs
    res, tmap, std, poses, weight = MRC.run(obs, rig)
    ids, C, s2 = MCR.map_rig_cov(obs, rig, MRC.TAG, tmap, poses, weight, int(res["world_id"]))
    check(ids, C, s2, res, tmap, std)


def test_huber_weights_and_the_inlier_variance_factor():
    obs, _, _, dist, bad = MBC.repair_cases()["small_swap"]
    res, tmap, std, poses, weight = MBC.run(obs, dist)
    assert res["n_soft"] > 0 and all(weight[f, s] < 1 for f, s in bad)
    ids, C, s2 = MCR.map_cov(obs, MBC.K, dist, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]), huber_px=MBC.HUBER)
    check(ids, C, s2, res, tmap, std)
    plain = MCR.map_cov(obs, MBC.K, dist, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]))[1]
    assert np.abs(np.sqrt(np.diag(plain)) / np.sqrt(np.diag(C)) - 1).max() > 1e-3                  # the weights matter


def test_tags_are_correlated():
    """what a per-tag std cannot say: the blocks between tags are far from zero"""
    obs, _, _ = MBC.noisy_block(6, 8)
    res, tmap, std, poses, weight = MBC.run(obs, None, huber=0.0)
    ids, C, _ = MCR.map_cov(obs, MBC.K, None, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]))
    d = np.sqrt(np.diag(C))
    Cn = C / np.outer(d, d)
    off = max(np.abs(Cn[6 * a:6 * a + 6, 6 * b:6 * b + 6]).max() for a in range(len(ids)) for b in range(a))
    assert off > 0.5, off


def test_nothing_to_report():
    obs, _, _ = MC.exact_block(4, K=K)
    res, tmap, std, poses, weight = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER)
    ids, C, s2 = MCR.map_cov(obs, K, None, LC.TAG_INNER, tmap, poses, np.zeros_like(weight), int(res["world_id"]))
    assert ids == [] and C.shape == (0, 0) and s2 == 0.0


def test_from_slots():
    slot = np.array([-1, 0, -1, 1, 2, -1], dtype=np.int32)
    M = np.arange(24.0 * 24).reshape(24, 24)
    ids, C = MCR.from_slots(slot, M)
    assert ids == [1, 3, 4] and np.array_equal(C, M[:18, :18])
    with pytest.raises(AssertionError):
        MCR.from_slots(np.array([1, 0], dtype=np.int32), M)
