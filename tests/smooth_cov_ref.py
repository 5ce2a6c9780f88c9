"""NumPy statement of the covariance of the smoothed sequence poses (asl_smooth_cov_frames_device / asl_smooth_cov_batch,
k_smooth_cov in aprilslam_amd/csrc/k_smooth.inc).  It is the definition the kernel is compared with.

The smoother (smooth_ref.py) minimises sum_f |r_f|^2 / sigma_px^2 + sum_f |m_f|^2, which is already whitened by sigma_px,
sigma_rot and sigma_trans.  So the covariance of the stacked left updates (w, v) of all frames is A^-1, A the undamped
block-tridiagonal matrix of smooth_ref.Problem.blocks at the returned poses: no sigma^2 factor, no estimate from the
residuals.  A frame's marginal is the diagonal block Sigma_ff of A^-1 (the other frames are not held fixed).

Block Cholesky by smooth_ref.block_factor, the forward pass of smooth_ref.tridiag_solve, with lam = 0 and no right-hand side: S_f = D_f - M_{f-1} M_{f-1}^T = L_f L_f^T, M_f = C_f L_f^-T, then back

    Sigma_{n-1} = L_{n-1}^-T L_{n-1}^-1
    Sigma_f     = L_f^-T (I + M_f^T Sigma_{f+1} M_f) L_f^-1        f = n - 2 ... 0

which is the selected inverse of a block-tridiagonal matrix (from A^-1 = L^-T L^-1 of the whole factor, one block column at
a time).  The operations run in the kernel's order: T = Sigma_{f+1} M_f and X = I + M_f^T T summed over k = 0, 1, ...;
L^T Z = X by columns, L^T Y^T = Z^T by rows; the lower triangle of Y, mirrored, is Sigma_f (the carry of the next step too).

The blocks are those of the one smooth_ref.Problem, so frame times and a rig come with it: smooth_cov / problem_blocks are
the single-camera front, smooth_rig_cov / rig_problem_blocks the rig's (T = world<-rig), over cov_records / blocks_at.

The record is the project's asl_pose_cov of a world<-camera pose (pose_cov_ref.convention_map(R_f, t_f, True)):
C_f = A_f Sigma_ff A_f^T, A_f = blockdiag(-R_f^T, -R_f^T); computed as R^T . R on every 3x3 block (the sign drops out), lower
triangle mirrored, so it is symmetric to the bit.  sigma_px: the given one.  dof: 8 (taking-part slots of all frames) - 6 =
8 sum n_tags + 6 (n - 1) residuals - 6 n unknowns, the same in every record.  status 0 ok; 1 the solve has none (smooth result
status != 0, i.e. frame status 1 or 4): zeros, dof 0; 2 A is not positive definite: zeros in EVERY frame, the inverse being
global -- a pivot p of column c of S_f needs p > 0 and p > PIVOT_TOL D_f[c][c] (pose_cov_ref.positive_definite's rule).
Test infrastructure, as smooth_ref.py is.
"""
import numpy as np

import pose_cov_ref as PC
import smooth_ref as SR
from aprilslam_amd._lib import POSE_COV_DTYPE


def pivot_rule(p, d):
    """the covariance's pivot rule against d, the undamped D_f's diagonal entry (pose_cov_ref.positive_definite's)"""
    return p > 0 and p > PC.PIVOT_TOL * d


def back_solve(L, iv, b):
    """x of L^T x = b"""
    x = np.zeros(6)
    for a in range(5, -1, -1):
        s = b[a]
        for k in range(a + 1, 6):
            s -= L[k, a] * x[k]
        x[a] = s * iv[a]
    return x


def mirror_lower(Y):
    return np.tril(Y) + np.tril(Y, -1).T


def marginals(D, C):
    """(n, 6, 6) diagonal blocks of A^-1 by the recursion, or None: A is not positive definite"""
    fac = SR.block_factor(D, C, pivot=pivot_rule)
    if fac is None:
        return None
    L, inv, M, _ = fac
    n = len(D)
    Sig = np.zeros((n, 6, 6))
    for f in range(n - 1, -1, -1):
        X = np.eye(6)
        if f + 1 < n:
            T, Q = np.zeros((6, 6)), np.zeros((6, 6))
            for k in range(6):
                T = T + np.outer(Sig[f + 1][:, k], M[f][k, :])
            for k in range(6):
                Q = Q + np.outer(M[f][k, :], T[k, :])
            X = X + Q
        Z = np.stack([back_solve(L[f], inv[f], X[:, c]) for c in range(6)], axis=1)
        Y = np.stack([back_solve(L[f], inv[f], Z[r, :]) for r in range(6)], axis=0)
        Sig[f] = mirror_lower(Y)
    return Sig


def to_record_convention(Sigma, R):
    """A Sigma A^T, A = blockdiag(-R^T, -R^T), in the kernel's order: U = Sigma diag(R, R), then diag(R, R)^T U"""
    U, Cv = np.zeros((6, 6)), np.zeros((6, 6))
    for b in (0, 3):
        U[:, b:b + 3] = (Sigma[:, b:b + 1] * R[0] + Sigma[:, b + 1:b + 2] * R[1]) + Sigma[:, b + 2:b + 3] * R[2]
    for b in (0, 3):
        Cv[b:b + 3, :] = (R[0][:, None] * U[b] + R[1][:, None] * U[b + 1]) + R[2][:, None] * U[b + 2]
    return mirror_lower(Cv)


def blocks_at(pb, poses):
    """(problem, the poses solved for, D, C) of a smooth_ref.Problem relinearised at the poses of a smooth output (huber_px >
    0: the weighted normal equations, a down-weighted corner contributing wgt of its information)"""
    P = [SR.pose_of_seed(p) for p in poses]
    D, C, _ = pb.blocks(pb.linearise(P))
    return pb, P, D, C


def problem_blocks(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px=0.0, times=None):
    """blocks_at of one camera's problem"""
    return blocks_at(SR.problem(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, times=times, huber_px=huber_px), poses)


def rig_problem_blocks(obs, tag_map, rig, tag_size, poses, sigma_px, sigma_rot, sigma_trans, times=None, huber_px=0.0):
    """blocks_at of a rig's problem"""
    return blocks_at(SR.rig_problem(obs, tag_map, rig, tag_size, sigma_px, sigma_rot, sigma_trans, times=times, huber_px=huber_px), poses)


def records(n, cov, sigma_px, dof, status):
    out = np.zeros(n, dtype=POSE_COV_DTYPE)
    out["cov"] = cov
    out["sigma_px"] = sigma_px
    out["dof"] = dof
    out["status"] = status
    return out


def cov_records(pb, poses, result, sigma_px):
    """the covariance records of the poses and result record of any smooth output (the statement's or the device's) of the
    smooth_ref.Problem pb -> ((n_frames,) POSE_COV_DTYPE, the assembled matrix A or None)"""
    n = len(poses)
    if int(result["status"]) != SR.OK:
        return records(n, 0.0, sigma_px, 0, PC.STATUS_NO_POSE), None
    _, P, D, C = blocks_at(pb, poses)
    dof = 8 * int(pb.n_tags.sum()) - 6
    Sig = marginals(D, C) if np.all(np.isfinite(D)) and np.all(np.isfinite(C)) else None
    if Sig is None:
        return records(n, 0.0, sigma_px, dof, PC.STATUS_NOT_PD), None
    return records(n, np.stack([to_record_convention(Sig[f], P[f][0]) for f in range(n)]), sigma_px, dof, PC.STATUS_OK), SR.dense(D, C)


def smooth_cov(obs, tag_map, K, dist, tag_size, poses, result, sigma_px, sigma_rot, sigma_trans, huber_px=0.0, times=None):
    """cov_records of one camera's output, T = world<-camera"""
    return cov_records(SR.problem(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, times=times, huber_px=huber_px),
                       poses, result, sigma_px)


def smooth_rig_cov(obs, tag_map, rig, tag_size, poses, result, sigma_px, sigma_rot, sigma_trans, times=None, huber_px=0.0):
    """cov_records of a rig's output, T = world<-rig"""
    return cov_records(SR.rig_problem(obs, tag_map, rig, tag_size, sigma_px, sigma_rot, sigma_trans, times=times, huber_px=huber_px),
                       poses, result, sigma_px)


def dense_marginals(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px=0.0):
    """the independent second route: (covariances (n, 6, 6) from np.linalg.inv of the assembled matrix, that matrix)"""
    pb, P, D, C = problem_blocks(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px)
    A = SR.dense(D, C)
    Ai = np.linalg.inv(A)
    out = np.zeros((len(poses), 6, 6))
    for f in range(len(poses)):
        Am = PC.convention_map(P[f][0], P[f][1], True)
        Cf = Am @ Ai[6 * f:6 * f + 6, 6 * f:6 * f + 6] @ Am.T
        out[f] = 0.5 * (Cf + Cf.T)
    return out, A


def min_pivot_ratio(D, C):
    """the smallest pivot / diagonal entry of the undamped factorisation (how far a case is from status 2)"""
    worst, Mp = np.inf, None
    for f in range(len(D)):
        S = np.array(D[f], dtype=np.float64)
        if Mp is not None:
            S = S - Mp @ Mp.T
        L = np.linalg.cholesky(S)
        worst = min(worst, float(np.min(np.diag(L) ** 2 / np.diag(D[f]))))
        Mp = np.linalg.solve(L, C[f].T).T if f + 1 < len(D) else None
    return worst


def position_std(cov):
    """|sqrt(diag C[3:])| per frame"""
    c = np.asarray(cov, dtype=np.float64).reshape(-1, 6, 6)
    return np.sqrt(np.einsum("nii->ni", c)[:, 3:].sum(axis=1))
