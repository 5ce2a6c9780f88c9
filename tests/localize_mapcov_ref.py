"""NumPy statement of the pose covariance of a localisation that carries the uncertainty of its map
(asl_localize_mapcov_*, asl_localize_rig_mapcov_*; loc_map_term in aprilslam_amd/csrc/k_localize.inc), over a slot model of
localize_ref (OneCamera) or rig_ref (RigModel), at a GIVEN pose and active set: localize_ref.solve_frame states the solve.

At the returned pose (R, t) = body<-world (the camera, or the rig), for a corner X of slot s, tag j(s), seen by camera c
at the body point Pb = R X + t, with Jr = d uv / d Pb (the projection's Jacobian; a rig: J_proj Re_c):

  J_s   8 x 6, the rows the solver forms over its left update of the pose:          Jr [-[Pb]x | I]
  M_s   8 x 6, the same residuals over the tag's (omega, v), a left update of world<-tag in the world frame (the
        convention of the map's tag_std and joint covariance):                       (Jr R) [-[X]x | I]
  A = sum J_s^T J_s,  N_s = J_s^T M_s
  Q = sum over the slots s, s' whose tag has a block, N_s Sigma_map[j(s), j(s')] N_s'^T     (a tag without one is exact)
  C = sigma^2 A^-1 + A^-1 Q A^-1, in the solver's (w, v); the record holds Amap C Amap^T, pose_cov_ref.convention_map's
      world<-body (r, d), with sigma, dof and statuses 1 and 2 as pose_cov_ref.cov_from_normal has them.
  status 3 (zeros): a cov_slot entry of an active slot outside [-1, n_blocks), or a block read that is not finite.

To first order the minimiser moves by -A^-1 (J^T e + sum_s N_s d_j(s)) under corner noise e and map errors d, which are
independent: the two terms of C.  tests/test_localize_mapcov_ref.py checks that against a Monte Carlo experiment."""
import numpy as np

import localize_ref as LR
import pose_cov_ref as PC
from aprilslam_amd._lib import POSE_COV_DTYPE

STATUS_BAD_MAP_COV = 3


def body_jacobian(model, Pb, ci):
    """(d uv / d Pb (n, 2, 3), in front (n,)) of the body points Pb (n, 3) seen by the cameras ci (n,)"""
    n = len(Pb)
    Jr, ok = np.zeros((n, 2, 3)), np.zeros(n, dtype=bool)
    if hasattr(model, "table"):                                  # rig_ref.RigModel
        for c, (cam, Re, te) in enumerate(model.table):
            m = np.flatnonzero(ci == c)
            if not len(m):
                continue
            P = Pb[m] @ Re.T + te
            f = P[:, 2] > LR.Z_MIN
            if f.any():
                Jr[m[f]] = LR.project(cam, P[f], jac=True)[1] @ Re
                ok[m[f]] = True
    else:                                                        # localize_ref.OneCamera
        f = Pb[:, 2] > LR.Z_MIN
        if f.any():
            Jr[f] = LR.project(model.cam, Pb[f], jac=True)[1]
            ok[f] = True
    return Jr, ok


def slot_rows(model, R, t, Xw, ci):
    """(J (n_slots, 8, 6), M (n_slots, 8, 6)) at the pose (R, t) for the corners Xw (4 n_slots, 3) of the cameras ci; a corner
    behind its camera has zero rows"""
    Pb = Xw @ R.T + t
    Jr, ok = body_jacobian(model, Pb, ci)
    Jr = Jr * ok[:, None, None]
    J = np.concatenate([Jr @ LR.neg_skew(Pb), Jr], axis=2)
    a = Jr @ R
    M = np.concatenate([a @ LR.neg_skew(Xw), a], axis=2)
    return J.reshape(-1, 8, 6), M.reshape(-1, 8, 6)


def pose_cov(model, R, t, Xw, uv, ci, slot_ids, sigma_px, cov_slot, map_cov):
    """The covariance of world<-body for the pose (R, t) over the active slots (their corners Xw, uv, ci as
    localize_ref.frame_points gives them, slot_ids their tag ids): (cov 6x6, sigma_px used, dof, status).
    cov_slot (n_ids,) and map_cov as asl_mapcov_* write them (any leading dimension: the matrix as a 2-D array)"""
    cost, H, _ = model.linearise(R, t, Xw, uv, ci)
    cov, sig, dof, status = PC.cov_from_normal(H, cost, len(Xw), R, t, float(sigma_px), True)
    if status != PC.STATUS_OK:
        return cov, sig, dof, status
    map_cov = np.asarray(map_cov, dtype=np.float64)
    nb = map_cov.shape[1] // 6
    k = np.array([int(cov_slot[i]) for i in slot_ids], dtype=np.int64)
    if ((k < -1) | (k >= nb)).any():
        return np.zeros((6, 6)), sig, dof, STATUS_BAD_MAP_COV
    use = np.flatnonzero(k >= 0)
    if not len(use):
        return cov, sig, dof, status
    J, M = slot_rows(model, R, t, Xw, ci)
    N = np.einsum('sri,srj->sij', J, M)[use]
    idx = (6 * k[use][:, None] + np.arange(6)[None, :]).ravel()
    S = map_cov[np.ix_(idx, idx)]
    if not np.isfinite(S).all():
        return np.zeros((6, 6)), sig, dof, STATUS_BAD_MAP_COV
    Nall = np.concatenate(list(N), axis=1)                       # 6 x 6 n
    Q = Nall @ S @ Nall.T
    G = PC.convention_map(R, t, True) @ np.linalg.inv(H)
    E = G @ Q @ G.T
    return cov + 0.5 * (E + E.T), sig, dof, status


def frame_cov(model, rows, tag_map, tag_size, Rt, active, sigma_px, cov_slot, map_cov):
    """localize_ref.frame_cov with the map's covariance: the POSE_COV_DTYPE record of solve_frame's pose Rt over its active
    (flat) slots; status 1 without a pose"""
    rec = np.zeros((), dtype=POSE_COV_DTYPE)
    rec["sigma_px"], rec["status"] = sigma_px, PC.STATUS_NO_POSE
    if Rt is not None:
        Xw, uv, ci = LR.frame_points(model, rows, tag_map, tag_size, active)
        ids = [int(rows.reshape(-1)["id"][s]) for s in active]
        rec["cov"], rec["sigma_px"], rec["dof"], rec["status"] = pose_cov(model, Rt[0], Rt[1], Xw, uv, ci, ids, sigma_px, cov_slot, map_cov)
    return rec


def normal_matrix(model, R, t, Xw, uv, ci):
    """the pose's J^T J (for the tests' condition number)"""
    return model.linearise(R, t, Xw, uv, ci)[1]
