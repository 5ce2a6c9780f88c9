"""NumPy statement of the rig mounting calibration (asl_calibrate_rig_frames_device / asl_calibrate_rig_batch,
aprilslam_amd/csrc/k_rigcal.inc): the same seed, connectivity rule, joint Levenberg-Marquardt schedule, frame-list sums and
covariance, on the host.  Test infrastructure, as calib_ref.py is for the camera calibration.

Input: obs (n_cams, n_frames, max_tags) asl_obs records, camera-major, a tag map (sizes through localize_ref.tag_half) and
n_cams asl_rig_camera records whose E = camera_c<-rig are the INITIAL mountings.  Unknowns: the mountings of the solved
cameras (6 each) and one pose rig<-world per used frame.

  seed        rig_ref.localize(obs, map, rig, tag_size): every frame under the initial mountings, the gate off.
  take part   mask(f): the cameras with a taking-part slot (flags & 1, a valid map entry) in frame f; only frames whose seed
              status is 0 count.  reach = {0}; n_cams - 1 sweeps over the frames in order, a frame with |mask| >= 2 whose
              mask meets reach joins its mask to reach.  Used frames: |mask| >= 2 and mask inside reach.  Solved cameras:
              reach without camera 0, in camera order.  Camera 0 is the gauge, a camera outside reach is held.
  model       P_r = R X + t, P_c = Re_c P_r + te_c, residual project_c(P_c) - pixel.  Left updates: the rig pose
              (R, t) <- (Rod(w) R, Rod(w) t + v), rows Jp Re_c [-[P_r]x | I] (rig_ref.py); the mounting
              (Re_c, te_c) <- (Rod(w_c) Re_c, Rod(w_c) te_c + v_c), rows Jp [-[P_c]x | I].  A corner with P_c.z <= Z_MIN costs
              BEHIND_COST and has no rows.
  joint LM    calib_ref.calibrate's schedule: per used frame U (6x6) and, per solved camera of its mask, W_c = J_rig^T J_c,
              V_c = J_c^T J_c, g_c; damped H + lambda diag(H); the frame eliminates its pose:
              S = sum_f (blockdiag(V) - W^T U^-1 W), b = sum_f (g - W^T U^-1 g_pose); S d = -b (Cholesky),
              d_pose_f = -U_f^-1 (g_pose_f + W_f d).  lambda0 = 1e-3, x10 after a rejected (or unsolvable) trial, x0.1 after
              an accepted one, at most max_iters trials; an accepted trial whose cost decrease is below 1e-12 of the cost
              before it ends the solve.  The frames' shares are summed over the list of used frames in LIST_CHUNKS
              contiguous chunks, each in order, then the chunks in order (cal_list_sum of k_calib.inc).
  at the end  the undamped S; sigma^2 = cost / dof, dof = 2 n_corners - 6 n_used - 6 n_solved (sigma_px^2 if sigma_px > 0);
              camera c's covariance is its block of sigma^2 S^-1, moved to the (r, d) convention of asl_pose_cov for the pose
              E_c: A = [I 0; -[te_c]x I], C = A C_(w,v) A^T, the lower triangle mirrored (symmetric to the bit).
  status      0 ok; 1 nothing to solve (no solved camera, or dof <= 0); 3 failed (non-finite state, or the undamped S
              not positive definite).  With 1 or 3 the rig comes back as given and every covariance has status 1.
  cameras     cam_status 0 solved, 1 the reference camera, 2 held; cam_frames: the used frames with the camera in the mask.
  frames      used: the refined pose (world<-rig), status 0, final rms_px, rms_seed_px / seed_slot of the seed, n_tags the
              taking-part slots; others: the seed's record, status 5 where that was 0.  Status 1: no frame is refined (all
              are "others"); status 3: the used frames keep the seed's record with status 4.
"""
import numpy as np

import localize_ref as LR
import rig_ref as RR
from aprilslam_amd._lib import POSE_COV_DTYPE, RIG_CALIB_RESULT_DTYPE, RIG_CAMERA_DTYPE

LAMBDA0 = 1e-3
REL_STOP = 1e-12
LIST_CHUNKS = 16
CAM_SOLVED, CAM_REFERENCE, CAM_HELD = 0, 1, 2
FRAME_OUTSIDE, FRAME_FAILED = 5, 4


def rig_records(rig):
    rec = rig.as_records() if hasattr(rig, "as_records") else rig
    return np.ascontiguousarray(rec, dtype=RIG_CAMERA_DTYPE).ravel()


def connect(masks, n_cams):
    """masks: per frame the set of cameras with a taking-part slot (empty for a frame whose seed failed) ->
    (reach, the used frames in order)"""
    reach = {0}
    for _ in range(n_cams - 1):
        for m in masks:
            if len(m) >= 2 and m & reach:
                reach |= m
    return reach, [f for f, m in enumerate(masks) if len(m) >= 2 and m <= reach]


def list_sum(rows):
    """cal_list_sum: the rows (n, ...) in LIST_CHUNKS contiguous chunks, each summed in order, then the chunks in order"""
    n = len(rows)
    chunk = (n + LIST_CHUNKS - 1) // LIST_CHUNKS
    total = np.zeros_like(rows[0])
    for q in range(LIST_CHUNKS):
        acc = np.zeros_like(rows[0])
        for k in range(q * chunk, min(n, (q + 1) * chunk)):
            acc = acc + rows[k]
        total = total + acc
    return total


def linearise(cams, E, col, R, t, Xw, uv, ci):
    """One frame at the rig pose (R, t) and the mountings E [(Re, te)]: (cost, U, g_pose, W (ns, 6, 6), V (ns, 6, 6),
    g (ns, 6)); col[c]: camera c's place among the solved ones, -1 if it is not solved"""
    ns = max(col) + 1
    U, gp = np.zeros((6, 6)), np.zeros(6)
    W, V, g = np.zeros((ns, 6, 6)), np.zeros((ns, 6, 6)), np.zeros((ns, 6))
    cost = 0.0
    Pr = Xw @ R.T + t
    for c in sorted(set(ci.tolist())):
        m = ci == c
        Re, te = E[c]
        P = Pr[m] @ Re.T + te
        ok = P[:, 2] > LR.Z_MIN
        cost += LR.BEHIND_COST * float((~ok).sum())
        if not ok.any():
            continue
        p, pr = P[ok], Pr[m][ok]
        q, Jp = LR.project(cams[c], p, jac=True)
        r = (q - uv[m][ok]).reshape(-1)
        cost += float(r @ r)
        Jr = Jp @ Re
        Jrig = np.concatenate([Jr @ LR.neg_skew(pr), Jr], axis=2).reshape(-1, 6)
        U += Jrig.T @ Jrig
        gp += Jrig.T @ r
        if col[c] >= 0:
            Jm = np.concatenate([Jp @ LR.neg_skew(p), Jp], axis=2).reshape(-1, 6)
            W[col[c]] += Jrig.T @ Jm
            V[col[c]] += Jm.T @ Jm
            g[col[c]] += Jm.T @ r
    return cost, U, gp, W, V, g


def schur(lins, lam):
    """the reduced system (S, b) over the solved cameras and per frame (U^-1 W, U^-1 g_pose), or None if a Cholesky fails"""
    shares, back = [], []
    for _, U, gp, W, V, g in lins:
        ns = len(W)
        Ud = U.copy()
        Ud[np.diag_indices(6)] *= 1 + lam
        Wf = np.concatenate(list(W), axis=1)                      # 6 x 6 ns
        Vf = np.zeros((6 * ns, 6 * ns))
        for j in range(ns):
            Vf[6 * j:6 * j + 6, 6 * j:6 * j + 6] = V[j]
        Vf[np.diag_indices(6 * ns)] *= 1 + lam
        try:
            L = np.linalg.cholesky(Ud)
        except np.linalg.LinAlgError:
            return None
        UW = np.linalg.solve(L.T, np.linalg.solve(L, Wf))
        Ug = np.linalg.solve(L.T, np.linalg.solve(L, gp))
        shares.append(np.concatenate([(Vf - Wf.T @ UW).ravel(), g.ravel() - Wf.T @ Ug]))
        back.append((UW, Ug))
    tot = list_sum(np.array(shares))
    p = 6 * len(lins[0][3])
    return tot[:p * p].reshape(p, p), tot[p * p:], back


def update(R, t, d):
    dR = LR.rodrigues(d[:3])
    return dR @ R, dR @ t + d[3:]


def convention(te):
    """A with (r, d) = A (w, v) for the pose E = (Re, te) itself (pose_cov_ref.convention_map, camera<-X)"""
    A = np.eye(6)
    A[3:, :3] = -np.array([[0.0, -te[2], te[1]], [te[2], 0.0, -te[0]], [-te[1], te[0], 0.0]])
    return A


def mirrored_lower(C):
    return np.tril(C) + np.tril(C, -1).T


def frame_points(model, obs, tag_map, tag_size, f):
    """(taking-part flat slots, Xw, uv, camera per corner) of frame f"""
    _, part, _ = LR.gather(obs[:, f], tag_map)
    if not part:
        return part, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, dtype=np.int64)
    return (part,) + LR.frame_points(model, obs[:, f], tag_map, tag_size, part)


def calibrate(obs, tag_map, rig, tag_size, max_iters=30, sigma_px=0.0, details=None):
    """-> (rig_out (n_cams,) RIG_CAMERA_DTYPE, result RIG_CALIB_RESULT_DTYPE, cov (n_cams,) POSE_COV_DTYPE,
    poses (n_frames,) CAM_POSE_DTYPE world<-rig).  details (a dict, optional) receives the undamped reduced matrix "S",
    the solved cameras "solved", the used frames "used" and the seed's poses "seed"."""
    obs = np.asarray(obs)
    assert obs.ndim == 3
    rec = rig_records(rig)
    n_cams, n_frames = obs.shape[0], obs.shape[1]
    assert len(rec) == n_cams
    sigma_px = float(sigma_px or 0.0)
    model = RR.RigModel(rec)
    cams = [tb[0] for tb in model.table]
    E = [(tb[1], tb[2]) for tb in model.table]

    seed = RR.localize(obs, tag_map, rec, tag_size)
    poses = seed.copy()
    pts = [frame_points(model, obs, tag_map, tag_size, f) for f in range(n_frames)]
    masks = [set(p[3].tolist()) if seed["status"][f] == 0 else set() for f, p in enumerate(pts)]
    reach, used = connect(masks, n_cams)
    solved = sorted(reach - {0})
    col = [solved.index(c) if c in solved else -1 for c in range(n_cams)]

    res = np.zeros((), dtype=RIG_CALIB_RESULT_DTYPE)
    cov = np.zeros(n_cams, dtype=POSE_COV_DTYPE)
    cov["status"] = 1
    cov["sigma_px"] = sigma_px
    res["sigma_px"] = sigma_px
    for c in range(n_cams):
        res["cam_status"][c] = CAM_REFERENCE if c == 0 else CAM_SOLVED if c in reach else CAM_HELD
        res["cam_frames"][c] = sum(1 for f in used if c in masks[f])
    n_corners = 4 * sum(len(pts[f][0]) for f in used)
    dof = 2 * n_corners - 6 * len(used) - 6 * len(solved)
    res["n_frames_used"], res["n_corners"], res["n_solved"] = len(used), n_corners, len(solved)
    poses["status"][seed["status"] == 0] = FRAME_OUTSIDE
    if details is not None:
        details.update(solved=solved, used=used, seed=seed, S=None)
    if not solved or dof <= 0:
        res["status"] = 1
        return rec.copy(), res, cov, poses

    state = []
    for f in used:
        T = seed["T"][f]
        R = T[:3, :3].T.copy()
        state.append((R, -(R @ T[:3, 3])))

    def lin_all(E_, st):
        return [linearise(cams, E_, col, R, t, *pts[f][1:]) for (R, t), f in zip(st, used)]

    lins = lin_all(E, state)
    cost = float(list_sum(np.array([l[0] for l in lins])))
    res["rms_init_px"] = np.sqrt(cost / n_corners)
    lam, iters = LAMBDA0, 0
    for _ in range(max_iters):
        iters += 1
        sys_ = schur(lins, lam)
        d = None
        if sys_ is not None:
            S, b, back = sys_
            try:
                L = np.linalg.cholesky(S)
                d = np.linalg.solve(L.T, np.linalg.solve(L, -b))
            except np.linalg.LinAlgError:
                d = None
        if d is None:
            lam *= 10
            continue
        E_n = list(E)
        for j, c in enumerate(solved):
            E_n[c] = update(E[c][0], E[c][1], d[6 * j:6 * j + 6])
        st_n = [update(R, t, -(Ug + UW @ d)) for (R, t), (UW, Ug) in zip(state, back)]
        lins_n = lin_all(E_n, st_n)
        cn = float(list_sum(np.array([l[0] for l in lins_n])))
        if cn < cost:
            stop = cost - cn < REL_STOP * cost
            E, state, lins, cost = E_n, st_n, lins_n, cn
            lam *= 0.1
            if stop:
                break
        else:
            lam *= 10
    res["iterations"] = iters

    def fail():
        res["status"] = 3
        for f in used:
            poses["status"][f] = FRAME_FAILED
        return rec.copy(), res, cov, poses

    if not (np.isfinite(cost) and all(np.all(np.isfinite(Re)) and np.all(np.isfinite(te)) for Re, te in E)):
        return fail()
    fin = schur(lins, 0.0)
    if fin is None:
        return fail()
    S = fin[0]
    try:
        np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return fail()
    if details is not None:
        details["S"] = S
    s2 = sigma_px * sigma_px if sigma_px > 0 else cost / dof
    sig = sigma_px if sigma_px > 0 else float(np.sqrt(s2))
    Sinv = np.linalg.inv(S)
    out = rec.copy()
    res["rms_px"] = np.sqrt(cost / n_corners)
    res["sigma_px"] = sig
    cov["sigma_px"] = sig
    for j, c in enumerate(solved):
        Re, te = E[c]
        out["E"][c] = np.c_[Re, te]
        A = convention(te)
        cov["cov"][c] = mirrored_lower(s2 * (A @ Sinv[6 * j:6 * j + 6, 6 * j:6 * j + 6] @ A.T))
        cov["dof"][c] = dof
        cov["status"][c] = 0
    for (R, t), l, f in zip(state, lins, used):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
        poses["T"][f] = T
        poses["rms_px"][f] = np.sqrt(l[0] / (4 * len(pts[f][0])))
        poses["n_tags"][f] = len(pts[f][0])
        poses["n_rejected"][f] = 0
        poses["status"][f] = 0
    return out, res, cov, poses


def solution_normal(obs, tag_map, rig_out, tag_size, result, poses):
    """The linearisation at a returned solution (the mountings of rig_out, the poses of the frames with status 0):
    (per used frame linearise()'s tuple, the mountings [(Re, te)], the solved cameras, cost, n_corners)"""
    obs = np.asarray(obs)
    rec = rig_records(rig_out)
    model = RR.RigModel(rec)
    cams = [tb[0] for tb in model.table]
    E = [(tb[1], tb[2]) for tb in model.table]
    solved = [c for c in range(1, len(rec)) if result["cam_status"][c] == CAM_SOLVED]
    col = [solved.index(c) if c in solved else -1 for c in range(len(rec))]
    lins, n_corners = [], 0
    for f in np.flatnonzero(poses["status"] == 0):
        _, Xw, uv, ci = frame_points(model, obs, tag_map, tag_size, f)
        T = poses["T"][f]
        R = T[:3, :3].T.copy()
        lins.append(linearise(cams, E, col, R, -(R @ T[:3, 3]), Xw, uv, ci))
        n_corners += len(Xw)
    return lins, E, solved, float(list_sum(np.array([l[0] for l in lins]))), n_corners


def _camera_covs(Minv_blocks, E, solved, s2):
    return {c: mirrored_lower(s2 * (convention(E[c][1]) @ B @ convention(E[c][1]).T)) for c, B in zip(solved, Minv_blocks)}


def _sigma2(sigma_px, cost, n_corners, n_frames, n_solved):
    return sigma_px * sigma_px if sigma_px and sigma_px > 0 else cost / (2 * n_corners - 6 * n_frames - 6 * n_solved)


def schur_cov(obs, tag_map, rig_out, tag_size, result, poses, sigma_px=0.0):
    """The covariances of calibrate() formed at a returned solution, through the Schur route: ({camera: 6x6}, the undamped
    reduced matrix S)"""
    lins, E, solved, cost, n_corners = solution_normal(obs, tag_map, rig_out, tag_size, result, poses)
    S = schur(lins, 0.0)[0]
    Sinv = np.linalg.inv(S)
    s2 = _sigma2(sigma_px, cost, n_corners, len(lins), len(solved))
    return _camera_covs([Sinv[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(len(solved))], E, solved, s2), S


def full_normal_cov(obs, tag_map, rig_out, tag_size, result, poses, sigma_px=0.0):
    """The same covariances from a dense inverse of the full (6 F + 6 n_solved) normal matrix at the solution (a check of
    the Schur route): ({camera: 6x6}, the full normal matrix)"""
    lins, E, solved, cost, n_corners = solution_normal(obs, tag_map, rig_out, tag_size, result, poses)
    F, p = len(lins), 6 * len(solved)
    H = np.zeros((6 * F + p, 6 * F + p))
    for k, (_, U, _, W, V, _) in enumerate(lins):
        sl = slice(6 * k, 6 * k + 6)
        H[sl, sl] = U
        for j in range(len(solved)):
            sj = slice(6 * F + 6 * j, 6 * F + 6 * j + 6)
            H[sl, sj] = W[j]
            H[sj, sl] = W[j].T
            H[sj, sj] += V[j]
    Hinv = np.linalg.inv(H)
    s2 = _sigma2(sigma_px, cost, n_corners, F, len(solved))
    return _camera_covs([Hinv[6 * F + 6 * j:6 * F + 6 * j + 6, 6 * F + 6 * j:6 * F + 6 * j + 6] for j in range(len(solved))], E, solved, s2), H


def mounting_error(E, T_true):
    """(degrees, units) of a 3x4 mounting E against the true 4x4 camera<-rig"""
    E = np.asarray(E, dtype=np.float64).reshape(3, 4)
    dR = E[:, :3] @ T_true[:3, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:, 3] - T_true[:3, 3]))
