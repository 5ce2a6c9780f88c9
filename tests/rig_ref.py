"""NumPy statement of the rig localisation (asl_localize_rig_frames_device / asl_localize_rig_batch,
aprilslam_amd/csrc/k_rig.inc), on top of localize_ref.py: the same gather, seed order, candidate rule, LM schedule, gate
and covariance, in the kernel's order of decisions.  Test infrastructure.

A rig of n_cams cameras; camera c has its own model (K_c, dist_c) and a fixed mounting E_c = camera_c<-rig.  The unknown of
a frame is rig<-world = (R, t).  For a world corner X seen by camera c at (iu, iv):

    P_r = R X + t,   P_c = Re_c P_r + te_c,   residual project_c(P_c) - (iu, iv)

and with the left update (R, t) <- (Rod(w) R, Rod(w) t + v) the Jacobian is J_proj_c(P_c) Re_c [-[P_r]x | I].

Per frame (obs[c][f] for every camera c: n_cams x max_tags records, global slot g = c * max_tags + s):

  gather   as localize_ref over the global slots (flags & 1, mapped id); one tag_size for the rig
  seed     the <= 8 global slots with flags & 2 of largest corner area (pixels squared as they are; ties: lower global
           slot), in global-slot order, plain then mirrored; a candidate of camera c is rig<-world = inv(E_c) (T_obs
           inv(map[id])) = (Re^T R_k, Re^T (t_k - te)); scored over ALL taking-part corners of ALL cameras, strictly lowest wins
  refine   localize_ref.lm with the rig linearisation
  gate     as localize_ref over global slots (at most 8 drops, never the last slot)
  output   T = world<-rig; counts over all cameras; status 1 (no mapped tag in any camera) / 2 (no seeding slot);
           seed_slot = global slot of the winner (+256 if mirrored)
  cov      pose_cov_ref.cov_from_normal of the rig normal matrix at the final pose over the slots still active,
           world<-rig convention, dof = 8 n_used - 6; mountings and map taken as exact
"""
import numpy as np

import localize_ref as LR
import pose_cov_ref as PC
from aprilslam_amd._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, RIG_CAMERA_DTYPE


def rig_table(rig):
    """[(localize_ref camera tuple, Re 3x3, te 3)] of RIG_CAMERA_DTYPE records (or a rig.Rig)"""
    rec = rig.as_records() if hasattr(rig, "as_records") else np.asarray(rig, dtype=RIG_CAMERA_DTYPE).ravel()
    out = []
    for r in rec:
        E = np.asarray(r["E"], dtype=np.float64).reshape(3, 4)
        out.append((LR.camera(r["K"], r["dist"][:r["n_dist"]]), E[:, :3].copy(), E[:, 3].copy()))
    return out


def corner_costs(table, R, t, Xw, uv, ci):
    """squared pixel error per corner (ci: its camera); BEHIND_COST at P_c.z <= Z_MIN"""
    Pr = Xw @ R.T + t
    e = np.full(len(Pr), LR.BEHIND_COST)
    for c, (cam, Re, te) in enumerate(table):
        m = ci == c
        if not m.any():
            continue
        P = Pr[m] @ Re.T + te
        ok = P[:, 2] > LR.Z_MIN
        if ok.any():
            r = LR.project(cam, P[ok]) - uv[m][ok]
            idx = np.flatnonzero(m)[ok]
            e[idx] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    return e


def linearise(table, R, t, Xw, uv, ci):
    """(cost, H, g) over the corners in their order: localize_ref.linearise with J_proj Re for J_proj and -[P_r]x"""
    Pr = Xw @ R.T + t
    n = len(Pr)
    J = np.zeros((n, 2, 6))
    r = np.zeros((n, 2))
    behind = np.ones(n, dtype=bool)
    for c, (cam, Re, te) in enumerate(table):
        m = ci == c
        if not m.any():
            continue
        P = Pr[m] @ Re.T + te
        ok = P[:, 2] > LR.Z_MIN
        if not ok.any():
            continue
        idx = np.flatnonzero(m)[ok]
        p = Pr[idx]
        q, Jp = LR.project(cam, P[ok], jac=True)
        Jr = Jp @ Re
        neg_px = np.zeros((len(p), 3, 3))           # -[P_r]x
        neg_px[:, 0, 1], neg_px[:, 0, 2] = p[:, 2], -p[:, 1]
        neg_px[:, 1, 0], neg_px[:, 1, 2] = -p[:, 2], p[:, 0]
        neg_px[:, 2, 0], neg_px[:, 2, 1] = p[:, 1], -p[:, 0]
        J[idx] = np.concatenate([Jr @ neg_px, Jr], axis=2)
        r[idx] = q - uv[idx]
        behind[idx] = False
    cost = LR.BEHIND_COST * float(behind.sum())
    H, g = np.zeros((6, 6)), np.zeros(6)
    if not behind.all():
        Jf, rf = J[~behind].reshape(-1, 6), r[~behind]
        cost += float((rf * rf).sum())
        H = Jf.T @ Jf
        g = Jf.T @ rf.reshape(-1)
    return cost, H, g


def rig_lin(table, Xw, uv, ci):
    """localize_ref.lm's lin over a frame's corners"""
    def lin(R, t, want):
        if want:
            return linearise(table, R, t, Xw, uv, ci)
        return float(corner_costs(table, R, t, Xw, uv, ci).sum()), None, None
    return lin


def _gather(rows, tag_map, tag_size):
    """rows (n_cams, max_tags) -> (flat records over global slots, taking-part global slots, seeding ones)"""
    flat = rows.reshape(-1)
    n_ids = len(tag_map)
    part = [g for g, o in enumerate(flat) if (o["flags"] & 1) and 0 <= o["id"] < n_ids and tag_map["valid"][o["id"]]]
    seeds = [g for g in part if flat["flags"][g] & 2]
    return flat, part, seeds


def frame_points(rows, tag_map, tag_size, slots):
    """world corners (4n, 3), image corners (4n, 2) and camera per corner (4n,) of the given global slots of one frame"""
    flat = rows.reshape(-1)
    Xw, uv = PC.frame_points(flat, tag_map, tag_size, slots)
    ci = np.repeat(np.asarray(slots, dtype=np.int64) // rows.shape[1], 4)
    return Xw, uv, ci


def seed_candidates(flat, max_tags, tag_map, table, seeds, Xw, uv, ci):
    """[(R, t, seed code, score)] in candidate order"""
    out = []
    for g in [seeds[k] for k in LR.top_k([LR.corner_area(flat["corners"][g]) for g in seeds])]:
        To = flat["T"][g].reshape(3, 4)
        M = tag_map["T"][flat["id"][g]].reshape(3, 4)
        _, Re, te = table[g // max_tags]
        for m in (0, 1):
            Ro, to = To[:, :3], To[:, 3]
            if m:
                Ro, to = LR.mirrored(Ro, to)
            Rk = Ro @ M[:, :3].T                    # camera<-world = T_obs inv(map)
            tk = to - Rk @ M[:, 3]
            Rc, tc = Re.T @ Rk, Re.T @ (tk - te)    # rig<-world = inv(E) of it
            out.append((Rc, tc, g + LR.MIRRORED * m, float(corner_costs(table, Rc, tc, Xw, uv, ci).sum())))
    return out


def candidate_scores(rows, tag_map, rig, tag_size):
    """{seed code: score} of one frame's candidates (for a choice between candidates that tie to rounding)"""
    table = rig_table(rig)
    flat, part, seeds = _gather(rows, tag_map, tag_size)
    if not seeds:
        return {}
    Xw, uv, ci = frame_points(rows, tag_map, tag_size, part)
    return {code: c for _, _, code, c in seed_candidates(flat, rows.shape[1], tag_map, table, seeds, Xw, uv, ci)}


def localize_frame(rows, tag_map, table, tag_size, gate, sigma_px=None, trace=None):
    """one frame's (n_cams, max_tags) asl_obs records -> (CAM_POSE_DTYPE record, POSE_COV_DTYPE record or None);
    trace (a dict, optional) receives "dropped" (global slots the gate dropped, in order) and "active" (those in the
    final solve)"""
    out = np.zeros((), dtype=CAM_POSE_DTYPE)
    out["T"] = np.eye(4)
    out["seed_slot"] = -1
    cov = None
    if sigma_px is not None:
        cov = np.zeros((), dtype=POSE_COV_DTYPE)
        cov["sigma_px"], cov["status"] = sigma_px, PC.STATUS_NO_POSE
    max_tags = rows.shape[1]
    flat, part, seeds = _gather(rows, tag_map, tag_size)
    if trace is not None:
        trace["dropped"], trace["active"] = [], []
    if not part or not seeds:
        out["status"] = 1 if not part else 2
        return out, cov
    Xw, uv, ci = frame_points(rows, tag_map, tag_size, part)
    best, best_cost = None, np.inf
    for Rc, tc, code, c in seed_candidates(flat, max_tags, tag_map, table, seeds, Xw, uv, ci):
        if c < best_cost:
            best, best_cost = (Rc, tc, code), c
    if best is None:
        out["status"] = 2
        return out, cov
    R, t, code = best
    n_part = len(part)
    R, t, cost = LR.lm(rig_lin(table, Xw, uv, ci), R, t)
    n_used, n_rej = n_part, 0
    active = np.ones(n_part, dtype=bool)
    if gate > 0:
        while n_rej < LR.MAX_GATE_DROPS and n_used > 1:
            e = corner_costs(table, R, t, Xw, uv, ci).reshape(-1, 4)
            rms = np.where(active, np.sqrt(((e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])) / 4), -1.0)
            worst = int(np.argmax(rms))                 # the first of equal maxima: the lower global slot
            if not rms[worst] > gate:
                break
            active[worst] = False
            if trace is not None:
                trace["dropped"].append(part[worst])
            n_rej += 1
            n_used -= 1
            keep = np.repeat(active, 4)
            R, t, cost = LR.lm(rig_lin(table, Xw[keep], uv[keep], ci[keep]), R, t)
    if trace is not None:
        trace["active"] = [g for g, a in zip(part, active) if a]
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -(R.T @ t)
    out["T"] = T
    out["rms_px"] = np.sqrt(cost / (4 * n_used))
    out["rms_seed_px"] = np.sqrt(best_cost / (4 * n_part))
    out["n_tags"] = n_used
    out["n_rejected"] = n_rej
    out["status"] = 0
    out["seed_slot"] = code
    if cov is not None:
        keep = np.repeat(active, 4)
        C, sig, dof, status = pose_cov(table, R, t, Xw[keep], uv[keep], ci[keep], sigma_px)
        cov["cov"], cov["sigma_px"], cov["dof"], cov["status"] = C, sig, dof, status
    return out, cov


def pose_cov(table, R, t, Xw, uv, ci, sigma_px):
    """(cov 6x6 of world<-rig, sigma used, dof, status) at rig<-world = (R, t) over the given corners"""
    cost, H, _ = linearise(table, R, t, Xw, uv, ci)
    return PC.cov_from_normal(H, cost, len(Xw), R, t, float(sigma_px), True)


def localize(obs, tag_map, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None, traces=None):
    """obs (n_cams, n_frames, max_tags) asl_obs records, camera-major -> (n_frames,) CAM_POSE_DTYPE, world<-rig; with
    sigma_px not None also (n_frames,) POSE_COV_DTYPE; traces (a list, optional) receives every frame's trace"""
    obs = np.asarray(obs)
    assert obs.ndim == 3
    table = rig_table(rig)
    assert len(table) == obs.shape[0]
    poses, covs = [], []
    for f in range(obs.shape[1]):
        tr = {} if traces is not None else None
        p, c = localize_frame(obs[:, f], tag_map, table, tag_size, float(max_tag_rms_px), sigma_px, tr)
        poses.append(p)
        covs.append(c)
        if traces is not None:
            traces.append(tr)
    poses = np.array(poses, dtype=CAM_POSE_DTYPE)
    if sigma_px is None:
        return poses
    return poses, np.array(covs, dtype=POSE_COV_DTYPE)
