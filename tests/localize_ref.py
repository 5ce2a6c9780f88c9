"""NumPy statement of the localisation against a tag map, for one camera (asl_localize_frames_device / asl_localize_batch)
and for a rig (asl_localize_rig_frames_device / asl_localize_rig_batch; the rig model is in rig_ref.py), with their
covariance forms: the same gather, candidate order, tie-break, Levenberg-Marquardt schedule and outlier gate as
loc_solve_frame<COV, Model> of aprilslam_amd/csrc/k_localize.inc (LocRig: k_rig.inc), frame by frame on the host.  Test infrastructure, as
oracle/gn_oracle.py is for the pose-graph LM.

Layout: the camera model and the pose primitives (camera .. lm), the slot model of one camera (OneCamera), and the one
frame solve over a slot model (gather .. localize_frames) with the covariance step (frame_cov, through
pose_cov_ref.cov_from_normal; pose_cov_ref imports nothing from here).  A slot model says three things, as LocOneCam and
LocRig do on the device:

  slot_camera(slot, max_tags)       the camera a flat slot belongs to
  costs / linearise(R, t, Xw, uv, ci)   squared pixel error per corner / (cost, H, g) at the pose solved for (ci: camera per corner)
  pose(Rk, tk, camera)              the pose solved for, of a slot's candidate camera<-world = (Rk, tk)

OneCamera costs every corner through its one camera and hands the candidate through: the pose solved for is camera<-world.

Per frame (n_cams x max_tags asl_obs records, n_cams = 1 for one camera; flat slot g = camera * max_tags + slot) against a map
of world<-tag poses indexed by id:

  size     a map entry's half side h (map_tag_half, aprilslam_amd/csrc/k_localize.inc; tag_half here, the one place
           under tests/ that states it): size == 0: the tag has the call's tag_size, h = half = float32(tag_size / 2);
           size > 0 and finite: the tag's own side, h = float32(size) * float32(0.5) (halving a float32 is exact);
           negative or not finite: the entry counts as valid = 0.
  gather   a slot takes part if flags & 1, 0 <= id < n_ids and map[id] is valid by the size rule; its 4 corners are 4
           residual pairs against the map tag's corners (object corners +-h of ITS tag, lb rb rt lt).  Every pass after
           the gather reads these points, so the refinement, the gate, the covariances and the sequence solves'
           linearisation state nothing about sizes.  A slot seeds candidates only if its PnP succeeded (flags & 2).
  seed     the <= 8 seeding slots of largest corner area (ties: lower slot), in slot order, each with its PnP pose and
           that pose's mirrored planar minimum: camera<-world = T_obs inv(map[id]), through the model's pose().  A
           record's PnP pose was solved at the call's tag_size: for a tag with a size of its own it has the right
           rotation and a translation short by half / h (scaling the object and the translation together leaves every
           ray where it is, under any lens), so both candidates are built from the translation times h / half
           (seed_translation; map_seed_scale of k_map.inc); a slot without a size keeps its translation's bytes.  Every
           candidate is scored by its total squared pixel error over ALL taking-part corners; the strictly lowest wins, so
           ties go to the lower slot and to the plain pose before the mirrored one.  seed_slot = slot (+256 if mirrored).
  refine   LM on the pose solved for, left update T <- [Rod(w) | v] T, delta = (w, v), analytic Jacobian
           dp_c/d delta = [-[p_c]x | I] through the camera model of k_pnp.inc (pinhole + 0 / 4 / 5 cv2 coefficients):
           at most 10 trial steps; (H + lambda diag(H)) delta = -g with lambda0 = 1e-3, x10 after a rejected step (or a
           failed Cholesky), x0.1 after an accepted one; an accepted step whose cost decrease is below 1e-12 of the
           cost before it ends the solve.  A corner at z <= 1e-9 costs 1e12 and adds nothing to H and g.
  gate     max_tag_rms_px > 0: after the solve, the slot with the largest own 4-corner RMS
           (sqrt(((e0 + e1) + (e2 + e3)) / 4), e = squared pixel distance of a corner; ties: lower slot) is dropped if
           that RMS exceeds the gate, and the solve runs again from the current pose; repeated while the worst slot of
           the new solve exceeds the gate, at most 8 times, and never down to no slot.  One slot at a time: a moved tag
           drags the first solve, and with it the residuals of its neighbours, over the gate as well.
  output   T = world<-camera (world<-rig) 4x4; rms_px = sqrt(cost / (4 n_tags)) of the final solve; rms_seed_px the same
           of the winning candidate over all taking-part slots; status 1 (no taking-part slot) / 2 (no seeding slot) leave
           T the identity, the counts 0 and seed_slot -1.
  cov      pose_cov_ref.cov_from_normal of the model's normal matrix at the final pose over the slots still active,
           world<-camera convention, dof = 8 n_used - 6; status 1 without a pose.
"""
import numpy as np

import pose_cov_ref as PC
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE

MAX_SEED_SLOTS = 8
LM_ITERS = 10
LAMBDA0 = 1e-3
REL_STOP = 1e-12
Z_MIN = 1e-9
BEHIND_COST = 1e12
MIRRORED = 256
MAX_GATE_DROPS = 8


def half_size(tag_size):
    return float(np.float32(tag_size / 2))


def size_half(size, tag_size):
    """the size rule on one asl_map_tag.size: (half side, whether it is the tag's own), or (None, False) for a bad size"""
    size = np.float32(size)
    if not (np.isfinite(size) and size >= 0):
        return None, False
    if size > 0:
        return float(size * np.float32(0.5)), True
    return half_size(tag_size), False


def tag_half(entry, tag_size):
    """size_half of one MAP_TAG_DTYPE entry; (None, False) also for valid == 0: an entry that does not take part"""
    return size_half(entry["size"], tag_size) if entry["valid"] else (None, False)


def seed_translation(t, h, own, tag_size):
    """the translation of a PnP pose solved at tag_size, as it is for a tag of half side h: times h / half for a tag with a
    size of its own, t itself otherwise"""
    return t * (h / half_size(tag_size)) if own else t


def half_corners(h):
    """the corners (lb rb rt lt) of a tag of half side h in its plane"""
    return np.array([[-h, -h], [h, -h], [h, h], [-h, h]], dtype=np.float64)


def object_corners(tag_size):
    return half_corners(half_size(tag_size))


def camera(K, dist):
    K = np.asarray(K, dtype=np.float64)
    d = (list(np.asarray(dist if dist is not None else [], dtype=np.float64).ravel()) + [0.0] * 5)[:5]
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + tuple(d)


def project(cam, P, jac=False):
    """pixel coordinates (n, 2) of camera-frame points P (n, 3), and d uv / d P (n, 2, 3): the formulas of project_dev"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    iz = 1 / P[:, 2]
    x, y = P[:, 0] * iz, P[:, 1] * iz
    r2 = x * x + y * y
    cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    dcd = k1 + r2 * (2 * k2 + 3 * k3 * r2)
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    uv = np.stack([fx * xd + cx, fy * yd + cy], axis=1)
    if not jac:
        return uv
    dxd_dx = cd + x * dcd * 2 * x + 2 * p1 * y + p2 * (2 * x + 4 * x)
    dxd_dy = x * dcd * 2 * y + 2 * p1 * x + p2 * 2 * y
    dyd_dx = y * dcd * 2 * x + p1 * 2 * x + 2 * p2 * y
    dyd_dy = cd + y * dcd * 2 * y + p1 * (2 * y + 4 * y) + 2 * p2 * x
    z0 = np.zeros_like(iz)
    dx_dP = np.stack([iz, z0, -x * iz], axis=1)
    dy_dP = np.stack([z0, iz, -y * iz], axis=1)
    J = np.empty((len(P), 2, 3))
    J[:, 0] = fx * (dxd_dx[:, None] * dx_dP + dxd_dy[:, None] * dy_dP)
    J[:, 1] = fy * (dyd_dx[:, None] * dx_dP + dyd_dy[:, None] * dy_dP)
    return uv, J


def rodrigues(r):
    """rodrigues_dev"""
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta < 2.220446049250313e-16:
        return np.eye(3)
    c, s = np.cos(theta), np.sin(theta)
    c1, it = 1 - c, 1 / theta
    x, y, z = r[0] * it, r[1] * it, r[2] * it
    return np.array([[c + c1 * x * x, c1 * x * y - s * z, c1 * x * z + s * y],
                     [c1 * x * y + s * z, c + c1 * y * y, c1 * y * z - s * x],
                     [c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z]])


def mirrored(R, t):
    """map_init.mirrored_pose of camera<-tag (R, t)"""
    s = t / np.sqrt(t @ t)
    Rs = 2.0 * np.outer(s, s) - np.eye(3)
    return Rs @ R @ np.diag([-1.0, -1.0, 1.0]), t.copy()


def corner_area(c8):
    """shoelace area of the float32 corners, in the kernel's operation order"""
    x = [float(c8[0]), float(c8[2]), float(c8[4]), float(c8[6])]
    y = [float(c8[1]), float(c8[3]), float(c8[5]), float(c8[7])]
    a = (x[0] * y[1] - x[1] * y[0]) + (x[1] * y[2] - x[2] * y[1]) + (x[2] * y[3] - x[3] * y[2]) + (x[3] * y[0] - x[0] * y[3])
    return 0.5 * abs(a)


def neg_skew(p):
    """-[p]x of every point of p (n, 3): d (Rod(w) p) / d w at w = 0"""
    S = np.zeros((len(p), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = p[:, 2], -p[:, 1]
    S[:, 1, 0], S[:, 1, 2] = -p[:, 2], p[:, 0]
    S[:, 2, 0], S[:, 2, 1] = p[:, 1], -p[:, 0]
    return S


def corner_costs(cam, R, t, Xw, uv):
    P = Xw @ R.T + t
    ok = P[:, 2] > Z_MIN
    e = np.full(len(P), BEHIND_COST)
    if ok.any():
        r = project(cam, P[ok]) - uv[ok]
        e[ok] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    return e


def linearise(cam, R, t, Xw, uv):
    P = Xw @ R.T + t
    ok = P[:, 2] > Z_MIN
    cost = BEHIND_COST * float((~ok).sum())
    H, g = np.zeros((6, 6)), np.zeros(6)
    if ok.any():
        p = P[ok]
        q, Jp = project(cam, p, jac=True)
        r = q - uv[ok]
        cost += float((r * r).sum())
        J = np.concatenate([Jp @ neg_skew(p), Jp], axis=2).reshape(-1, 6)
        H = J.T @ J
        g = J.T @ r.reshape(-1)
    return cost, H, g


def chol6_solve(A, b):
    """chol6_solve_tri_dev on the lower triangle; None if A is not positive definite"""
    L = np.zeros((6, 6))
    inv = np.zeros(6)
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                if not s > 0:
                    return None
                L[i, i] = np.sqrt(s)
                inv[i] = 1 / L[i, i]
            else:
                L[i, j] = s * inv[j]
    x = np.array(b, dtype=np.float64)
    for i in range(6):
        s = x[i]
        for k in range(i):
            s -= L[i, k] * x[k]
        x[i] = s * inv[i]
    for i in range(5, -1, -1):
        s = x[i]
        for k in range(i + 1, 6):
            s -= L[k, i] * x[k]
        x[i] = s * inv[i]
    return x


class OneCamera:
    """the slot model of one camera (LocOneCam): every slot is its own, and a candidate is handed through"""

    def __init__(self, cam):
        self.cam = cam

    def slot_camera(self, slot, max_tags):
        return 0

    def costs(self, R, t, Xw, uv, ci):
        return corner_costs(self.cam, R, t, Xw, uv)

    def linearise(self, R, t, Xw, uv, ci):
        return linearise(self.cam, R, t, Xw, uv)

    def pose(self, Rk, tk, camera):
        return Rk, tk


def model_lin(model, Xw, uv, ci):
    """lm's lin over a frame's corners: (cost, H, g) of the model's linearise, or (cost, None, None) for the trial cost alone"""
    def lin(R, t, want):
        if want:
            return model.linearise(R, t, Xw, uv, ci)
        return float(model.costs(R, t, Xw, uv, ci).sum()), None, None
    return lin


def corner_lin(cam, Xw, uv):
    """model_lin of one camera"""
    return model_lin(OneCamera(cam), Xw, uv, None)


def lm(lin, R, t):
    """the fixed schedule of the module docstring on (R, t), the left update R <- Rod(w) R, t <- Rod(w) t + v;
    lin(R, t, want) -> (cost, H, g), H and g only if want; returns (R, t, cost)"""
    cost, H, g = lin(R, t, True)
    lam = LAMBDA0
    for _ in range(LM_ITERS):
        A = H.copy()
        A[np.diag_indices(6)] += lam * np.diag(H)
        d = chol6_solve(A, -g)
        if d is None:
            lam *= 10
            continue
        dR = rodrigues(d[:3])
        Rn, tn = dR @ R, dR @ t + d[3:]
        cn = lin(Rn, tn, False)[0]
        if cn < cost:
            stop = cost - cn < REL_STOP * cost
            R, t, cost = Rn, tn, cn
            lam *= 0.1
            if stop:
                break
            cost, H, g = lin(R, t, True)
        else:
            lam *= 10
    return R, t, cost


def top_k(areas, k=MAX_SEED_SLOTS):
    """positions of the k largest areas (ties: lower position), in ascending position order"""
    order = sorted(range(len(areas)), key=lambda i: (-areas[i], i))
    return sorted(order[:k])


def _world_corners(M12, obj):
    M = np.asarray(M12, dtype=np.float64).reshape(3, 4)
    return np.stack([M[:, 0] * ox + M[:, 1] * oy + M[:, 3] for ox, oy in obj])


def tag_points(corners8, tag_size):
    """a tag's own corners (4, 3) in its frame and its image corners (4, 2)"""
    return np.c_[object_corners(tag_size), np.zeros(4)], np.asarray(corners8, dtype=np.float64).reshape(4, 2)


def gather(rows, tag_map):
    """one frame's records -> (the records over flat slots, the taking-part slots, the seeding ones)"""
    flat = rows.reshape(-1)
    n_ids = len(tag_map)
    part = [s for s, o in enumerate(flat) if (o["flags"] & 1) and 0 <= o["id"] < n_ids and tag_half(tag_map[o["id"]], 1.0)[0] is not None]
    seeds = [s for s in part if flat["flags"][s] & 2]
    return flat, part, seeds


def frame_points(model, rows, tag_map, tag_size, slots):
    """world corners (4n, 3), image corners (4n, 2) and camera per corner (4n,) of the given flat slots of one frame"""
    flat = rows.reshape(-1)
    Xw = np.concatenate([_world_corners(tag_map["T"][i], half_corners(tag_half(tag_map[i], tag_size)[0])) for i in flat["id"][list(slots)]])
    uv = np.concatenate([flat["corners"][s].astype(np.float64).reshape(4, 2) for s in slots])
    ci = np.repeat(np.array([model.slot_camera(s, rows.shape[-1]) for s in slots], dtype=np.int64), 4)
    return Xw, uv, ci


def seed_candidates(model, rows, tag_map, tag_size, seeds, Xw, uv, ci):
    """(the <= 8 seeding slots of largest area in slot order, [(R, t, seed code, score)] in candidate order: those slots,
    plain then mirrored, each from the slot's PnP pose at its tag's own half)"""
    flat = rows.reshape(-1)
    chosen = [seeds[k] for k in top_k([corner_area(flat["corners"][s]) for s in seeds])]
    out = []
    for s in chosen:
        To = flat["T"][s].reshape(3, 4)
        M = tag_map["T"][flat["id"][s]].reshape(3, 4)
        to0 = seed_translation(To[:, 3], *tag_half(tag_map[flat["id"][s]], tag_size), tag_size)
        for m in (0, 1):
            Ro, to = To[:, :3], to0
            if m:
                Ro, to = mirrored(Ro, to)
            Rk = Ro @ M[:, :3].T                    # camera<-world = T_obs inv(map)
            tk = to - Rk @ M[:, 3]
            Rc, tc = model.pose(Rk, tk, model.slot_camera(s, rows.shape[-1]))
            out.append((Rc, tc, s + MIRRORED * m, float(model.costs(Rc, tc, Xw, uv, ci).sum())))
    return chosen, out


def candidate_scores(model, rows, tag_map, tag_size):
    """{seed code: score} of one frame's candidates (for comparing a choice between candidates that tie to rounding)"""
    _, part, seeds = gather(rows, tag_map)
    if not seeds:
        return {}
    Xw, uv, ci = frame_points(model, rows, tag_map, tag_size, part)
    return {code: c for _, _, code, c in seed_candidates(model, rows, tag_map, tag_size, seeds, Xw, uv, ci)[1]}


def solve_frame(model, rows, tag_map, tag_size, gate):
    """one frame's asl_obs records, (max_tags,) or (n_cams, max_tags) -> (CAM_POSE_DTYPE record, the pose solved for (R, t)
    or None without one, the flat slots in the final solve, trace); trace: the chosen seeding slots in slot order
    ("top_k"), the slots the gate dropped in order ("dropped"), each gate round's own RMS per taking-part slot
    ("gate_rms") and the slots in the final solve ("active")"""
    out = np.zeros((), dtype=CAM_POSE_DTYPE)
    out["T"] = np.eye(4)
    out["seed_slot"] = -1
    trace = {"top_k": [], "dropped": [], "gate_rms": [], "active": []}
    _, part, seeds = gather(rows, tag_map)
    if not part or not seeds:
        out["status"] = 1 if not part else 2
        return out, None, [], trace
    Xw, uv, ci = frame_points(model, rows, tag_map, tag_size, part)
    trace["top_k"], cands = seed_candidates(model, rows, tag_map, tag_size, seeds, Xw, uv, ci)
    best, best_cost = None, np.inf
    for Rc, tc, code, c in cands:
        if c < best_cost:
            best, best_cost = (Rc, tc, code), c
    if best is None:
        out["status"] = 2
        return out, None, [], trace
    R, t, code = best
    n_part = len(part)
    R, t, cost = lm(model_lin(model, Xw, uv, ci), R, t)
    n_used, n_rej = n_part, 0
    active = np.ones(n_part, dtype=bool)
    if gate > 0:
        while n_rej < MAX_GATE_DROPS and n_used > 1:
            e = model.costs(R, t, Xw, uv, ci).reshape(-1, 4)
            rms = np.where(active, np.sqrt(((e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])) / 4), -1.0)
            worst = int(np.argmax(rms))                 # the first of equal maxima: the lower slot
            trace["gate_rms"].append(rms)
            if not rms[worst] > gate:
                break
            active[worst] = False
            trace["dropped"].append(part[worst])
            n_rej += 1
            n_used -= 1
            keep = np.repeat(active, 4)
            R, t, cost = lm(model_lin(model, Xw[keep], uv[keep], ci[keep]), R, t)
    trace["active"] = [s for s, a in zip(part, active) if a]
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
    return out, (R, t), trace["active"], trace


def pose_cov(model, R, t, Xw, uv, ci, sigma_px, world_from_camera=True):
    """Covariance of the pose (R, t) (reported for its inverse if world_from_camera) that minimises the model's pixel
    residuals of the points Xw (n, 3) seen at uv (n, 2) by the cameras ci (n,):
    (cov 6x6 in the order rx ry rz px py pz, sigma_px used, dof, status)"""
    cost, H, _ = model.linearise(R, t, Xw, uv, ci)
    return PC.cov_from_normal(H, cost, len(Xw), R, t, float(sigma_px), world_from_camera)


def frame_cov(model, rows, tag_map, tag_size, Rt, active, sigma_px):
    """the POSE_COV_DTYPE record of solve_frame's pose Rt over its active slots; status 1 without a pose"""
    cov = np.zeros((), dtype=POSE_COV_DTYPE)
    cov["sigma_px"], cov["status"] = sigma_px, PC.STATUS_NO_POSE
    if Rt is not None:
        Xw, uv, ci = frame_points(model, rows, tag_map, tag_size, active)
        cov["cov"], cov["sigma_px"], cov["dof"], cov["status"] = pose_cov(model, Rt[0], Rt[1], Xw, uv, ci, sigma_px)
    return cov


def localize_frames(model, frames, tag_map, tag_size, gate, sigma_px=None, traces=None):
    """solve_frame of every frame -> (n_frames,) CAM_POSE_DTYPE; with sigma_px not None also (n_frames,) POSE_COV_DTYPE;
    traces (a list, optional) receives every frame's trace"""
    poses, covs = [], []
    for rows in frames:
        out, Rt, active, trace = solve_frame(model, rows, tag_map, tag_size, float(gate))
        poses.append(out)
        if sigma_px is not None:
            covs.append(frame_cov(model, rows, tag_map, tag_size, Rt, active, sigma_px))
        if traces is not None:
            traces.append(trace)
    poses = np.array(poses, dtype=CAM_POSE_DTYPE)
    if sigma_px is None:
        return poses
    return poses, np.array(covs, dtype=POSE_COV_DTYPE)


def localize(obs, tag_map, K, dist, tag_size, max_tag_rms_px=0.0, sigma_px=None, traces=None):
    """obs (n_frames, max_tags) asl_obs records, tag_map (n_ids,) asl_map_tag records -> localize_frames of one camera,
    world<-camera"""
    obs = np.asarray(obs)
    if obs.ndim == 1:
        obs = obs[None]
    return localize_frames(OneCamera(camera(K, dist)), obs, tag_map, tag_size, max_tag_rms_px, sigma_px, traces)
