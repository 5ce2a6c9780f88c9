"""NumPy statement of locating unmapped tags from posed frames (asl_locate_tags_frames_device / asl_locate_tags_batch,
aprilslam_amd/csrc/k_locate.inc): the dual of localize_ref.py.  There a frame's camera pose is solved with the map held
fixed; here a tag's world<-tag pose G is solved from all its views with the cameras held fixed.  The result is not the
joint optimum: the frame poses are taken as exact, as localisation takes the map as exact.  Test infrastructure.

Inputs: obs (n_frames, max_tags) asl_obs records of one camera, poses (n_frames,) asl_cam_pose (T = world<-camera), a map
block (n_ids,) asl_map_tag, the camera model, tag_size, max_view_rms_px, min_views, optionally sigma_px.

  wanted   id i is solved for if map[i].valid == 0 and its size is >= 0 and finite; size > 0 is the tag's own side, 0 the
           call's tag_size (map_tag_half's rule on the size: localize_ref.size_half).  Valid entries, and invalid ones
           with a bad size, get status 1.
  views    frame f takes part if poses[f].status is 0 or 6 and rows 0..2 of its T are finite; in such a frame the first
           slot with flags & 1 and id == i is the view.  C_f = inv(T_f) = camera<-world, formed from the record as
           (R^T, -R^T p).  Fewer than min_views views: status 2.
  cost     over the active views' 4 corners: project(C_f (G X_q)) - uv, X_q = (+-h, +-h, 0), lb rb rt lt.  A corner at
           z <= 1e-9 costs 1e12 and adds no row.  Left update G <- [Rod(w) | v] G in the world frame:
           J = J_proj R_f [-[X_w]x | I].
  seed     the <= 8 active views with flags & 2 of largest corner area (ties: lower list position), walked in list order,
           plain before mirrored: G = inv(C_f) T_obs, a sized tag's PnP translation first times h_id / half
           (localize_ref.seed_translation), the mirror
           formed in the camera frame.  The strictly lowest total cost over all active views wins.  No seeding view, or
           every score NaN: status 3.
  refine   localize_ref.lm: 10 trials, lambda0 = 1e-3, stop on a relative decrease below 1e-12.
  gate     max_view_rms_px > 0: while the active view of largest own 4-corner RMS (ties: lower list position) exceeds the
           gate it is dropped, one at a time, at most 8, never below one view.  After each drop the solve is RE-SEEDED: the
           start is the lowest-cost of the current pose (candidate 0) and the candidates of the active seeding views, and
           the LM runs from there.  (Localisation continues from the current pose.  A spoiled view can pull the first solve
           into the tag's mirrored minimum; continuing from there left tags about 1 rad off at 0.4 to 0.7 px RMS, while the
           candidates of the remaining views, scored without the spoiled one, lead back.)
  output   map[i].T = G rows 0..2, valid = 1, size kept; every other entry keeps its bytes.  Per id a TAG_FIT_DTYPE record:
           rms_px = sqrt(cost / (4 n_views)) of the final solve, rms_seed_px the same of the winning first candidate over
           all views, n_views (status 2 and 3: the views found), n_rejected, status, seed_frame (-1 if none), seed_mirrored.
  cov      pose_cov_ref.cov_from_normal of the normal matrix at the pose written over the views still active, in the
           convention of the pose solved for itself (A = [I 0; -[p]x I] with p of G), dof = 8 n_views - 6; status 1 for an
           id not located.
"""
import numpy as np

import pose_cov_ref as PC
from aprilslam_amd._lib import MAP_TAG_DTYPE, POSE_COV_DTYPE, TAG_FIT_DTYPE
from localize_ref import (BEHIND_COST, MAX_GATE_DROPS, MAX_SEED_SLOTS, Z_MIN, camera, corner_area, lm, mirrored, neg_skew, project, seed_translation,
                          size_half, top_k)

STATUS_LOCATED, STATUS_NOT_WANTED, STATUS_FEW_VIEWS, STATUS_NO_PNP = 0, 1, 2, 3
FRAME_STATUSES = (0, 6)


def wanted_half(entry, tag_size):
    """(half side, whether it is the tag's own) of a map entry that is wanted: not mapped, with a good size; else (None, False)"""
    return size_half(entry["size"], tag_size) if entry["valid"] == 0 else (None, False)


def frame_ok(pose):
    return int(pose["status"]) in FRAME_STATUSES and bool(np.all(np.isfinite(pose["T"][:3])))


def views_of(obs, poses, i):
    """[(frame, slot)] of id i, in frame order"""
    out = []
    for f in range(len(obs)):
        if not frame_ok(poses[f]):
            continue
        hit = np.flatnonzero(((obs["flags"][f] & 1) != 0) & (obs["id"][f] == i))
        if len(hit):
            out.append((f, int(hit[0])))
    return out


def view_camera(pose):
    """C_f = (R, t) camera<-world of one asl_cam_pose"""
    T = np.asarray(pose["T"], dtype=np.float64)
    R = T[:3, :3].T
    return R, -(R @ T[:3, 3])


def tag_corners(h):
    return np.array([[-h, -h, 0.0], [h, -h, 0.0], [h, h, 0.0], [-h, h, 0.0]])


class TagViews:
    """the views of one tag: cameras (Rc (n, 3, 3), tc (n, 3)), image corners (n, 4, 2), the records' flags and PnP poses"""

    def __init__(self, cam, obs, poses, views, h, own, tag_size):
        self.cam, self.h, self.own, self.tag_size = cam, h, own, tag_size
        self.views = views
        cams = [view_camera(poses[f]) for f, _ in views]
        self.Rc = np.array([c[0] for c in cams]).reshape(-1, 3, 3)
        self.tc = np.array([c[1] for c in cams]).reshape(-1, 3)
        self.uv = np.array([obs["corners"][f, s].astype(np.float64).reshape(4, 2) for f, s in views]).reshape(-1, 4, 2)
        self.flags = [int(obs["flags"][f, s]) for f, s in views]
        self.To = [obs["T"][f, s].reshape(3, 4) for f, s in views]
        self.area = [corner_area(obs["corners"][f, s]) for f, s in views]
        self.obj = tag_corners(h)

    def _points(self, R, t, act):
        Xw = self.obj @ R.T + t                                              # (4, 3), the same for every view
        P = np.einsum("vij,qj->vqi", self.Rc[act], Xw) + self.tc[act][:, None, :]
        return Xw, P.reshape(-1, 3)

    def costs(self, R, t, act):
        """squared pixel error per corner (4 per active view) at world<-tag (R, t)"""
        _, P = self._points(R, t, act)
        ok = P[:, 2] > Z_MIN
        e = np.full(len(P), BEHIND_COST)
        if ok.any():
            r = project(self.cam, P[ok]) - self.uv[act].reshape(-1, 2)[ok]
            e[ok] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        return e

    def linearise(self, R, t, act):
        """(cost, H, g) of the left update of world<-tag over the active views"""
        Xw, P = self._points(R, t, act)
        ok = P[:, 2] > Z_MIN
        cost = BEHIND_COST * float((~ok).sum())
        H, g = np.zeros((6, 6)), np.zeros(6)
        if ok.any():
            q, Jp = project(self.cam, P[ok], jac=True)
            r = q - self.uv[act].reshape(-1, 2)[ok]
            cost += float((r * r).sum())
            Rc = np.repeat(self.Rc[act], 4, axis=0)[ok]                      # per corner
            Xall = np.tile(Xw, (int(act.sum()), 1))[ok]
            A = Jp @ Rc                                                      # d uv / d X_world
            J = np.concatenate([A @ neg_skew(Xall), A], axis=2).reshape(-1, 6)
            H = J.T @ J
            g = J.T @ r.reshape(-1)
        return cost, H, g

    def lin(self, act):
        def f(R, t, want):
            if want:
                return self.linearise(R, t, act)
            return float(self.costs(R, t, act).sum()), None, None
        return f

    def candidates(self, act):
        """[(R, t, list position, mirrored, score)] of the active seeding views, in candidate order"""
        seeds = [v for v in range(len(self.views)) if act[v] and (self.flags[v] & 2)]
        chosen = [seeds[k] for k in top_k([self.area[v] for v in seeds], MAX_SEED_SLOTS)]
        out = []
        for v in chosen:
            Ro, to = self.To[v][:, :3], seed_translation(self.To[v][:, 3], self.h, self.own, self.tag_size)
            Wr = self.Rc[v].T                                                # inv(C_f)
            Wt = -(Wr @ self.tc[v])
            for m in (0, 1):
                Rm, tm = mirrored(Ro, to) if m else (Ro, to)
                R, t = Wr @ Rm, Wr @ tm + Wt
                out.append((R, t, v, m, float(self.costs(R, t, act).sum())))
        return out


def solve_tag(tv, gate, min_views):
    """one tag's TagViews -> (TAG_FIT_DTYPE record, (R, t) of world<-tag or None, the active mask, trace); trace: the
    list positions the gate dropped in order ("dropped") and every first candidate's (position, mirrored, score) ("first")"""
    fit = np.zeros((), dtype=TAG_FIT_DTYPE)
    fit["seed_frame"] = -1
    n = len(tv.views)
    trace = {"dropped": [], "first": []}
    act = np.ones(n, dtype=bool)
    if n < min_views:
        fit["status"], fit["n_views"] = STATUS_FEW_VIEWS, n
        return fit, None, act, trace
    best, best_cost = None, np.inf
    for R, t, v, m, c in tv.candidates(act):
        trace["first"].append((v, m, c))
        if c < best_cost:
            best, best_cost = (R, t, v, m), c
    if best is None:
        fit["status"], fit["n_views"] = STATUS_NO_PNP, n
        return fit, None, act, trace
    R, t, v0, m0 = best
    first_cost = best_cost
    R, t, cost = lm(tv.lin(act), R, t)
    n_used, n_rej = n, 0
    if gate > 0:
        while n_rej < MAX_GATE_DROPS and n_used > 1:
            e = np.full((n, 4), 0.0)
            e[act] = tv.costs(R, t, act).reshape(-1, 4)
            rms = np.where(act, np.sqrt(((e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])) / 4), -1.0)
            worst = int(np.argmax(rms))                                      # the first of equal maxima
            if not rms[worst] > gate:
                break
            act[worst] = False
            trace["dropped"].append(worst)
            n_rej += 1
            n_used -= 1
            start, start_cost = (R, t), float(tv.costs(R, t, act).sum())     # candidate 0: the current pose
            for Rk, tk, _, _, c in tv.candidates(act):
                if c < start_cost:
                    start, start_cost = (Rk, tk), c
            R, t, cost = lm(tv.lin(act), start[0], start[1])
    fit["rms_px"] = np.sqrt(cost / (4 * n_used))
    fit["rms_seed_px"] = np.sqrt(first_cost / (4 * n))
    fit["n_views"], fit["n_rejected"], fit["status"] = n_used, n_rej, STATUS_LOCATED
    fit["seed_frame"], fit["seed_mirrored"] = tv.views[v0][0], m0
    return fit, (R, t), act, trace


def tag_cov(tv, Rt, act, sigma_px):
    """the POSE_COV_DTYPE record of solve_tag's pose over its active views; status 1 without a pose"""
    cov = np.zeros((), dtype=POSE_COV_DTYPE)
    cov["sigma_px"], cov["status"] = sigma_px, PC.STATUS_NO_POSE
    if Rt is not None:
        cost, H, _ = tv.linearise(Rt[0], Rt[1], act)
        C, cov["sigma_px"], cov["dof"], cov["status"] = PC.cov_from_normal(H, cost, 4 * int(act.sum()), Rt[0], Rt[1], float(sigma_px), False)
        cov["cov"] = np.tril(C) + np.tril(C, -1).T       # the lower triangle in both, as the kernel stores it: symmetric to the bit
    return cov


def locate_tags(obs, poses, map_records, K, dist, tag_size, max_view_rms_px=0.0, min_views=2, sigma_px=None, traces=None):
    """-> (the extended map (a copy), (n_ids,) TAG_FIT_DTYPE[, (n_ids,) POSE_COV_DTYPE if sigma_px is not None]);
    traces (a dict, optional) receives {id: (TagViews, trace, (R, t) or None, active mask)} of every wanted id"""
    obs = np.asarray(obs)
    if obs.ndim == 1:
        obs = obs[None]
    out = np.array(map_records, dtype=MAP_TAG_DTYPE).ravel().copy()
    cam = camera(K, dist)
    fits, covs = [], []
    for i in range(len(out)):
        h, own = wanted_half(out[i], tag_size)
        if h is None:
            fit = np.zeros((), dtype=TAG_FIT_DTYPE)
            fit["status"], fit["seed_frame"] = STATUS_NOT_WANTED, -1
            Rt, tv, act = None, None, None
        else:
            tv = TagViews(cam, obs, poses, views_of(obs, poses, i), h, own, tag_size)
            fit, Rt, act, trace = solve_tag(tv, float(max_view_rms_px), int(min_views))
            if traces is not None:
                traces[i] = (tv, trace, Rt, act)
        if Rt is not None:
            out["T"][i] = np.c_[Rt[0], Rt[1]].ravel()
            out["valid"][i] = 1
        fits.append(fit)
        if sigma_px is not None:
            covs.append(tag_cov(tv, Rt, act, sigma_px))
    fits = np.array(fits, dtype=TAG_FIT_DTYPE)
    if sigma_px is None:
        return out, fits
    return out, fits, np.array(covs, dtype=POSE_COV_DTYPE)
