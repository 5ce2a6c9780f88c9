"""Inputs the map-covariance localisation tests share (tests/test_localize_mapcov_ref.py on the CPU,
tests/test_gpu_localize_mapcov.py on the device): a synthetic joint covariance of a map -- independent per-tag errors plus an
error common to every tag, so that the blocks between tags are not zero -- and the map perturbed by a draw from it."""
import numpy as np

import localize_ref as LR

ROT_TAG, POS_TAG = 2e-3, 0.05        # per tag: rad and scene units, independent
ROT_COMMON, POS_COMMON = 1e-3, 0.03  # common to every tag


def synthetic_cov(ids):
    """(6 n, 6 n) covariance of the (omega, v) of the tags ids: diag(ROT_TAG^2, POS_TAG^2) per tag plus the common-mode term
    in every block"""
    n = len(ids)
    ind = np.diag([ROT_TAG ** 2] * 3 + [POS_TAG ** 2] * 3)
    com = np.diag([ROT_COMMON ** 2] * 3 + [POS_COMMON ** 2] * 3)
    return np.kron(np.eye(n), ind) + np.kron(np.ones((n, n)), com)


def cov_slot(ids, n_ids):
    slot = np.full(n_ids, -1, dtype=np.int32)
    slot[list(ids)] = np.arange(len(ids))
    return slot


def perturbed(records, ids, d):
    """the map records with tag ids[k] moved by the left update (omega, v) = d[6 k : 6 k + 6] in the world frame"""
    out = records.copy()
    for k, i in enumerate(ids):
        T = np.asarray(records["T"][i], dtype=np.float64).reshape(3, 4)
        dR = LR.rodrigues(d[6 * k:6 * k + 3])
        out["T"][i] = np.c_[dR @ T[:, :3], dR @ T[:, 3] + d[6 * k + 3:6 * k + 6]].ravel()
    return out


def random_spd(n, rng, scale=1e-3):
    """a well-conditioned dense covariance (n, n) with correlations everywhere"""
    B = rng.normal(size=(n, n))
    C = B @ B.T / n + np.eye(n)
    s = scale * (1 + rng.uniform(size=n))
    return C * np.outer(s, s)
