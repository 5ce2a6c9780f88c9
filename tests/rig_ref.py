"""NumPy statement of the rig localisation (asl_localize_rig_frames_device / asl_localize_rig_batch and their covariance
forms): the rig slot model (LocRig of aprilslam_amd/csrc/k_rig.inc) for the one frame solve of localize_ref.py, which
states the gather, seed order, candidate rule, LM schedule, gate and covariance.  Test infrastructure.

A rig of n_cams cameras; camera c has its own model (K_c, dist_c) and a fixed mounting E_c = camera_c<-rig.  The pose
solved for is rig<-world = (R, t).  For a world corner X seen by camera c at (iu, iv):

    P_r = R X + t,   P_c = Re_c P_r + te_c,   residual project_c(P_c) - (iu, iv)

and with the left update (R, t) <- (Rod(w) R, Rod(w) t + v) the Jacobian is J_proj_c(P_c) Re_c [-[P_r]x | I].

obs[c][f] for every camera c: n_cams x max_tags records per frame, flat slot g = c * max_tags + s, one tag_size for the
rig.  A candidate of camera c is rig<-world = inv(E_c) (T_obs inv(map[id])) = (Re^T R_k, Re^T (t_k - te)), scored over ALL
taking-part corners of ALL cameras.  T = world<-rig, counts over all cameras; mountings and map are taken as exact.
"""
import numpy as np

import localize_ref as LR
from aprilslam_amd._lib import RIG_CAMERA_DTYPE


def rig_table(rig):
    """[(localize_ref camera tuple, Re 3x3, te 3)] of RIG_CAMERA_DTYPE records (or a rig.Rig)"""
    rec = rig.as_records() if hasattr(rig, "as_records") else np.asarray(rig, dtype=RIG_CAMERA_DTYPE).ravel()
    out = []
    for r in rec:
        E = np.asarray(r["E"], dtype=np.float64).reshape(3, 4)
        out.append((LR.camera(r["K"], r["dist"][:r["n_dist"]]), E[:, :3].copy(), E[:, 3].copy()))
    return out


class RigModel:
    """the slot model of a rig over its rig_table"""

    def __init__(self, rig):
        self.table = rig_table(rig)

    def slot_camera(self, slot, max_tags):
        return slot // max_tags

    def pose(self, Rk, tk, camera):
        _, Re, te = self.table[camera]
        return Re.T @ Rk, Re.T @ (tk - te)          # rig<-world = inv(E) camera<-world

    def costs(self, R, t, Xw, uv, ci):
        """squared pixel error per corner (ci: its camera); BEHIND_COST at P_c.z <= Z_MIN"""
        Pr = Xw @ R.T + t
        e = np.full(len(Pr), LR.BEHIND_COST)
        for c, (cam, Re, te) in enumerate(self.table):
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

    def linearise(self, R, t, Xw, uv, ci):
        """(cost, H, g) over the corners in their order: localize_ref.linearise with J_proj Re for J_proj and -[P_r]x"""
        Pr = Xw @ R.T + t
        n = len(Pr)
        J = np.zeros((n, 2, 6))
        r = np.zeros((n, 2))
        behind = np.ones(n, dtype=bool)
        for c, (cam, Re, te) in enumerate(self.table):
            m = ci == c
            if not m.any():
                continue
            P = Pr[m] @ Re.T + te
            ok = P[:, 2] > LR.Z_MIN
            if not ok.any():
                continue
            idx = np.flatnonzero(m)[ok]
            q, Jp = LR.project(cam, P[ok], jac=True)
            Jr = Jp @ Re
            J[idx] = np.concatenate([Jr @ LR.neg_skew(Pr[idx]), Jr], axis=2)
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


def localize(obs, tag_map, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None, traces=None):
    """obs (n_cams, n_frames, max_tags) asl_obs records, camera-major -> localize_ref.localize_frames of the rig, world<-rig"""
    obs = np.asarray(obs)
    assert obs.ndim == 3
    model = RigModel(rig)
    assert len(model.table) == obs.shape[0]
    frames = [obs[:, f] for f in range(obs.shape[1])]
    return LR.localize_frames(model, frames, tag_map, tag_size, max_tag_rms_px, sigma_px, traces)
