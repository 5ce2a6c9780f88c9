"""NumPy statement of the first-order pose covariance (asl_pose_cov: asl_localize_cov_frames_device /
asl_localize_cov_batch in k_localize.inc, asl_pose_cov_device / asl_solve_pnp_cov_batch in k_posecov.inc).  It is the
definition the kernels are compared with.  Test infrastructure, as localize_ref.py is for the solver itself, which
imports this module: localize_ref.pose_cov applies cov_from_normal to a slot model's normal matrix.

The solvers refine camera<-X = (R, t) by the left update R <- Rod(w) R, t <- Rod(w) t + v and minimise the squared pixel
residuals of the corners; localize_ref.linearise gives their cost, H = J^T J and g in those coordinates (w, v).  At the
solution the Gauss-Newton covariance of (w, v) is sigma^2 H^-1.

The record reports the error of the pose T = [R_o | p] that is handed out as (r, d) with R_true = Rod(r) R_o and
p_true = p + d, which is (r, d) = A (w, v) to first order, so C = sigma^2 A H^-1 A^T:

  camera<-tag    T = (R, t) itself:  R_true = Rod(w) R                        ->  r = w
                                     t_true = Rod(w) t + v = t + w x t + v    ->  d = v - [t]x w
  world<-camera  T = (R^T, -R^T t):  R_o,true = (Rod(w) R)^T = Rod(-R^T w) R^T  ->  r = -R^T w
                                     p_true = -R^T Rod(-w) (Rod(w) t + v) = p - R^T v  ->  d = -R^T v

sigma: the given sigma_px if > 0, else sqrt(cost / dof), dof = 2 * corners - 6.  status 2 (zeros) if H is not positive
definite: a pivot of its Cholesky factorisation (the order and operations of chol6_solve_tri_dev) that is not above
PIVOT_TOL times its diagonal entry.  In Jacobi-scaled terms that pivot is 1 / (scaled H^-1)_ii >= 1 / kappa, so the
threshold only refuses matrices whose condition number has passed ~1e13, where float64 has no digit of the inverse left.
"""
import numpy as np

PIVOT_TOL = 1e-13
STATUS_OK, STATUS_NO_POSE, STATUS_NOT_PD = 0, 1, 2


def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def convention_map(R, t, world_from_camera):
    """A (6x6) with (r, d) = A (w, v) at camera<-X = (R, t)"""
    A = np.zeros((6, 6))
    if world_from_camera:
        A[:3, :3] = -R.T
        A[3:, 3:] = -R.T
    else:
        A[:3, :3] = np.eye(3)
        A[3:, :3] = -skew(t)
        A[3:, 3:] = np.eye(3)
    return A


def output_pose(R, t, world_from_camera):
    """(R_o, p) of the pose the covariance belongs to"""
    return (R.T, -(R.T @ t)) if world_from_camera else (R, t)


def positive_definite(H):
    """every pivot of the Cholesky factorisation above PIVOT_TOL of its diagonal entry"""
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = H[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                if not (s > 0 and s > PIVOT_TOL * H[i, i]):
                    return False
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return True


def scaled_condition(H):
    """2-norm condition number of the Jacobi-scaled H (unit diagonal)"""
    s = 1 / np.sqrt(np.diag(H))
    return float(np.linalg.cond(H * np.outer(s, s)))


def cov_from_normal(H, cost, n_corners, R, t, sigma_px, world_from_camera):
    """(cov 6x6, sigma_px used, dof, status) from the normal matrix and cost at camera<-X = (R, t)"""
    dof = 2 * int(n_corners) - 6
    s2 = sigma_px * sigma_px if sigma_px > 0 else cost / dof
    sig = float(sigma_px) if sigma_px > 0 else float(np.sqrt(s2))
    if not (np.all(np.isfinite(H)) and np.isfinite(s2) and positive_definite(H)):
        return np.zeros((6, 6)), sig, dof, STATUS_NOT_PD
    A = convention_map(R, t, world_from_camera)
    return s2 * (A @ np.linalg.inv(H) @ A.T), sig, dof, STATUS_OK


def no_pose(sigma_px):
    """status 1: the pose has no covariance"""
    return np.zeros((6, 6)), float(sigma_px), 0, STATUS_NO_POSE


def pose_error(R_est, p_est, R_true, p_true):
    """(r, d) of an estimate against the truth: Rod(r) = R_true R_est^T, d = p_true - p_est"""
    Q = R_true @ R_est.T
    w = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]]) / 2
    s = np.sqrt(w @ w)
    ang = np.arctan2(s, (np.trace(Q) - 1) / 2)
    r = w * (ang / s) if s > 1e-12 else w
    return np.concatenate([r, p_true - p_est])
