"""NumPy statement of locating unmapped tags from a camera rig's posed frames (asl_locate_tags_rig_frames_device /
asl_locate_tags_rig_batch, LocateRig of aprilslam_amd/csrc/k_locate.inc): the rig view model for the one tag solve of
locate_ref.py, which states wanted ids, seed order, candidate rule, LM schedule, gate with re-seeding, fit record and
covariance.  Test infrastructure.

Inputs: obs (n_cams, n_frames, max_tags) asl_obs records, camera-major, poses (n_frames,) asl_cam_pose with
T = world<-rig, a map block (n_ids,) asl_map_tag, the camera table (RIG_CAMERA_DTYPE records or a rig.Rig), tag_size,
max_view_rms_px, min_views, optionally sigma_px.

  views    frame f takes part under locate_ref.frame_ok.  In such a frame every camera c = 0..n_cams-1 gives at most one
           view of id i: its first slot with flags & 1 and id == i.  The same id in two cameras of a frame is two views.
           The list is in (frame, camera) order and min_views counts its entries.
  camera   of a view: C = E_c inv(T_f) = (Re R, Re t + te) with (R, t) = locate_ref.view_camera(poses[f]) and
           (Re, te) the mounting camera_c<-rig; its corners go through camera c's own model.
  seed     the <= 8 active views with flags & 2 of largest corner area, in pixels as they are (cameras of different focal
           length are not put on one scale), ties to the lower list position; G = inv(C) T_obs.
  output   locate_ref's; seed_frame is the frame of the winning first view.  dof = 8 n_views - 6; the mountings and the
           frame poses are taken as exact.

With one camera at the identity every number is locate_ref.locate_tags's: Re = I multiplies exactly.
"""
import numpy as np

import locate_ref as QR
from aprilslam_amd._lib import MAP_TAG_DTYPE, POSE_COV_DTYPE, TAG_FIT_DTYPE
from localize_ref import BEHIND_COST, Z_MIN, corner_area, neg_skew, project
from rig_ref import rig_table


def views_of(obs, poses, i):
    """[(frame, camera, slot)] of id i, in (frame, camera) order"""
    out = []
    for f in range(obs.shape[1]):
        if not QR.frame_ok(poses[f]):
            continue
        for c in range(obs.shape[0]):
            hit = np.flatnonzero(((obs["flags"][c, f] & 1) != 0) & (obs["id"][c, f] == i))
            if len(hit):
                out.append((f, c, int(hit[0])))
    return out


class TagViews(QR.TagViews):
    """the views of one tag over a rig: locate_ref.TagViews with a camera, a model and a (frame, camera, slot) per view;
    table: rig_ref.rig_table's.  solve_tag and tag_cov of locate_ref run on it as they are."""

    def __init__(self, table, obs, poses, views, h, own, tag_size):
        self.table, self.h, self.own, self.tag_size = table, h, own, tag_size
        self.views = views
        self.vcam = np.array([c for _, c, _ in views], dtype=np.int64)
        cams = []
        for f, c, _ in views:
            R, t = QR.view_camera(poses[f])                                  # rig<-world
            _, Re, te = table[c]
            cams.append((Re @ R, Re @ t + te))                               # camera_c<-world
        self.Rc = np.array([c[0] for c in cams]).reshape(-1, 3, 3)
        self.tc = np.array([c[1] for c in cams]).reshape(-1, 3)
        self.uv = np.array([obs["corners"][c, f, s].astype(np.float64).reshape(4, 2) for f, c, s in views]).reshape(-1, 4, 2)
        self.flags = [int(obs["flags"][c, f, s]) for f, c, s in views]
        self.To = [obs["T"][c, f, s].reshape(3, 4) for f, c, s in views]
        self.area = [corner_area(obs["corners"][c, f, s]) for f, c, s in views]
        self.obj = QR.tag_corners(h)

    def _project(self, P, ci, jac):
        """localize_ref.project of every point through the model of its own camera ci"""
        uv, J = np.zeros((len(P), 2)), np.zeros((len(P), 2, 3))
        for c in np.unique(ci):
            m = ci == c
            if jac:
                uv[m], J[m] = project(self.table[c][0], P[m], jac=True)
            else:
                uv[m] = project(self.table[c][0], P[m])
        return (uv, J) if jac else uv

    def costs(self, R, t, act):
        _, P = self._points(R, t, act)
        ci = np.repeat(self.vcam[act], 4)
        ok = P[:, 2] > Z_MIN
        e = np.full(len(P), BEHIND_COST)
        if ok.any():
            r = self._project(P[ok], ci[ok], False) - self.uv[act].reshape(-1, 2)[ok]
            e[ok] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        return e

    def linearise(self, R, t, act):
        Xw, P = self._points(R, t, act)
        ci = np.repeat(self.vcam[act], 4)
        ok = P[:, 2] > Z_MIN
        cost = BEHIND_COST * float((~ok).sum())
        H, g = np.zeros((6, 6)), np.zeros(6)
        if ok.any():
            q, Jp = self._project(P[ok], ci[ok], True)
            r = q - self.uv[act].reshape(-1, 2)[ok]
            cost += float((r * r).sum())
            Rc = np.repeat(self.Rc[act], 4, axis=0)[ok]
            Xall = np.tile(Xw, (int(act.sum()), 1))[ok]
            A = Jp @ Rc
            J = np.concatenate([A @ neg_skew(Xall), A], axis=2).reshape(-1, 6)
            H = J.T @ J
            g = J.T @ r.reshape(-1)
        return cost, H, g


def locate_tags_rig(obs, poses, map_records, rig, tag_size, max_view_rms_px=0.0, min_views=2, sigma_px=None, traces=None):
    """-> (the extended map (a copy), (n_ids,) TAG_FIT_DTYPE[, (n_ids,) POSE_COV_DTYPE if sigma_px is not None]);
    traces (a dict, optional) receives {id: (TagViews, trace, (R, t) or None, active mask)} of every wanted id"""
    obs = np.asarray(obs)
    assert obs.ndim == 3
    table = rig_table(rig)
    assert len(table) == obs.shape[0]
    out = np.array(map_records, dtype=MAP_TAG_DTYPE).ravel().copy()
    fits, covs = [], []
    for i in range(len(out)):
        h, own = QR.wanted_half(out[i], tag_size)
        if h is None:
            fit = np.zeros((), dtype=TAG_FIT_DTYPE)
            fit["status"], fit["seed_frame"] = QR.STATUS_NOT_WANTED, -1
            Rt, tv, act = None, None, None
        else:
            tv = TagViews(table, obs, poses, views_of(obs, poses, i), h, own, tag_size)
            fit, Rt, act, trace = QR.solve_tag(tv, float(max_view_rms_px), int(min_views))
            if traces is not None:
                traces[i] = (tv, trace, Rt, act)
        if Rt is not None:
            out["T"][i] = np.c_[Rt[0], Rt[1]].ravel()
            out["valid"][i] = 1
        fits.append(fit)
        if sigma_px is not None:
            covs.append(QR.tag_cov(tv, Rt, act, sigma_px))
    fits = np.array(fits, dtype=TAG_FIT_DTYPE)
    if sigma_px is None:
        return out, fits
    return out, fits, np.array(covs, dtype=POSE_COV_DTYPE)
