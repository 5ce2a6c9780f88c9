"""What the GPU tests of the pose solvers share (test_gpu_pose_cov.py, test_gpu_rig.py): the covariance bar and two small
conveniences.

Bound on a covariance, per element: |C_gpu - C_ref|_ij <= 600 eps kappa sqrt(C_ii C_jj), kappa the 2-norm condition
number of the Jacobi-scaled reference normal matrix (a backward-stable Cholesky inverse errs by a small multiple of
n eps kappa; 600 = 100 n).  Every compared pose must have 600 eps kappa <= 1e-6, which is asserted as well."""
import numpy as np

import pose_cov_ref as PC

EPS = np.finfo(np.float64).eps


def assert_cov_close(got, ref, H, what):
    kappa = PC.scaled_condition(H)
    tol = 600 * EPS * kappa
    assert tol <= 1e-6, (what, kappa)
    s = np.sqrt(np.diag(ref))
    err = np.abs(got - ref) / np.outer(s, s)
    assert err.max() <= tol, (what, err.max(), tol)
    assert np.array_equal(got, got.T), what


def dev_bytes(a, dev):
    """the bytes of a NumPy array on the device"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)


def rel(a, b):
    return abs(a - b) / max(1.0, abs(b))
