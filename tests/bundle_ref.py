"""NumPy statement of the tag-bundle calls (asl_localize_bundles_* and asl_bundle_relative_*; k_localize.inc's bundle
dimension and k_bundle.inc).  Test infrastructure.

Localisation: bundle b is a table of asl_map_tag records with T = bundle_b<-tag, and the pose of bundle b in frame f is
literally the one-map statement (localize_ref.localize, rig_ref.localize) of frame f with that table as its map, so
T = bundle_b<-camera (bundle_b<-rig).  Nothing else is stated here: the stack [f, b] of those calls.

The relative pose of bundle b in the frame of a reference bundle a, T_a = [R_a | p_a], T_b = [R_b | p_b]:

    T_ab = T_a inv(T_b):   R_ab = R_a R_b^T,   q = R_ab p_b,   p_ab = p_a - q

The covariances are in the (r, d) convention of asl_pose_cov (pose_cov_ref.py): R_true = Rod(r) R, p_true = p + d.  Then

    R_ab,true = Rod(r_a) R_ab Rod(-r_b) = Rod(r_a) Rod(-R_ab r_b) R_ab          ->  r_ab = r_a - R_ab r_b
    p_ab,true = p_a + d_a - Rod(r_ab) R_ab (p_b + d_b)                          ->  d_ab = d_a + [q]x r_ab - R_ab d_b

to first order, i.e. (r_ab, d_ab) = J_a (r_a, d_a) + J_b (r_b, d_b) with

    J_a = [I 0; [q]x I],   J_b = [-R_ab 0; -[q]x R_ab  -R_ab],   C_ab = J_a C_a J_a^T + J_b C_b J_b^T

the two poses taken as independent (their solves share no corner).  tests/test_bundle_ref.py checks both Jacobians
against central differences of the exact composition.

Statuses of a relative record: 0 ok; 1 bundle b or the reference has no pose (pose status != 0): identity, zeros; 2 both
posed but no covariances given or one of the two with status != 0: T valid, zeros.  b == ref: identity, zeros, 0 or 1 by
the reference's pose.
"""
import numpy as np

import localize_ref as LR
import rig_ref as RR
from aprilslam_amd._lib import BUNDLE_REL_DTYPE

REL_OK, REL_NO_POSE, REL_NO_COV = 0, 1, 2


def _stack(per_bundle, sigma_px):
    """[b] of (n_frames,) records (or pairs of them) -> (n_frames, n_bundles)"""
    if sigma_px is None:
        return np.stack(per_bundle, axis=1)
    return np.stack([p for p, _ in per_bundle], axis=1), np.stack([c for _, c in per_bundle], axis=1)


def localize_bundles(obs, tables, K, dist, tag_size, max_tag_rms_px=0.0, sigma_px=None):
    """obs (n_frames, max_tags) asl_obs, tables (n_bundles, n_ids) asl_map_tag -> (n_frames, n_bundles) CAM_POSE_DTYPE (and
    POSE_COV_DTYPE with sigma_px not None): localize_ref.localize once per bundle"""
    return _stack([LR.localize(obs, t, K, dist, tag_size, max_tag_rms_px, sigma_px) for t in tables], sigma_px)


def localize_bundles_rig(obs, tables, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None):
    """obs (n_cams, n_frames, max_tags): rig_ref.localize once per bundle"""
    return _stack([RR.localize(obs, t, rig, tag_size, max_tag_rms_px, sigma_px) for t in tables], sigma_px)


def skew(a, xp=np):
    return xp.array([[0 * a[0], -a[2], a[1]], [a[2], 0 * a[0], -a[0]], [-a[1], a[0], 0 * a[0]]])


def jacobians(Ta, Tb, dtype=np.float64):
    """(T_ab 4x4, J_a 6x6, J_b 6x6) at the poses Ta = ref<-camera and Tb = bundle<-camera, in dtype"""
    Ta, Tb = np.asarray(Ta, dtype=dtype), np.asarray(Tb, dtype=dtype)
    Rab = Ta[:3, :3] @ Tb[:3, :3].T
    q = Rab @ Tb[:3, 3]
    Tab = np.zeros((4, 4), dtype=dtype)
    Tab[:3, :3], Tab[:3, 3], Tab[3, 3] = Rab, Ta[:3, 3] - q, 1
    Q = skew(q).astype(dtype)
    Ja, Jb = np.zeros((6, 6), dtype=dtype), np.zeros((6, 6), dtype=dtype)
    Ja[:3, :3], Ja[3:, :3], Ja[3:, 3:] = np.eye(3, dtype=dtype), Q, np.eye(3, dtype=dtype)
    Jb[:3, :3], Jb[3:, :3], Jb[3:, 3:] = -Rab, -(Q @ Rab), -Rab
    return Tab, Ja, Jb


def relative(Ta, Ca, Tb, Cb, dtype=np.float64):
    """(T_ab, C_ab) of two posed bundles with their covariances; dtype np.longdouble is the second evaluation that the
    device tolerance is derived from (test_bundle_ref.py)"""
    Tab, Ja, Jb = jacobians(Ta, Tb, dtype)
    Ca, Cb = np.asarray(Ca, dtype=dtype), np.asarray(Cb, dtype=dtype)
    return Tab, Ja @ Ca @ Ja.T + Jb @ Cb @ Jb.T


def relative_records(poses, cov, ref):
    """poses (n_frames, n_bundles) CAM_POSE_DTYPE, cov as many POSE_COV_DTYPE or None -> (n_frames, n_bundles)
    BUNDLE_REL_DTYPE: the statement of asl_bundle_relative_batch with the status rules"""
    poses = np.asarray(poses)
    out = np.zeros(poses.shape, dtype=BUNDLE_REL_DTYPE)
    out["T"] = np.eye(4)
    for f in range(poses.shape[0]):
        a = poses[f, ref]
        for b in range(poses.shape[1]):
            p = poses[f, b]
            if a["status"] != 0 or p["status"] != 0:
                out["status"][f, b] = REL_NO_POSE
            elif b == ref:
                out["status"][f, b] = REL_OK
            elif cov is None or cov["status"][f, ref] != 0 or cov["status"][f, b] != 0:
                out["T"][f, b] = jacobians(a["T"], p["T"])[0]
                out["status"][f, b] = REL_NO_COV
            else:
                out["T"][f, b], out["cov"][f, b] = relative(a["T"], cov["cov"][f, ref], p["T"], cov["cov"][f, b])
    return out


def compose_exact(Ta, xa, Tb, xb):
    """The exact composition at perturbed poses, for the central differences: Ta moved by xa = (r_a, d_a) and Tb by xb in the
    convention above, T_ab of the moved poses, and its error (r_ab, d_ab) against T_ab of the poses as they are."""
    import pose_cov_ref as PC

    def moved(T, x):
        M = np.eye(4)
        M[:3, :3] = LR.rodrigues(np.asarray(x[:3], dtype=np.float64)) @ T[:3, :3]
        M[:3, 3] = T[:3, 3] + x[3:]
        return M
    T0 = np.asarray(Ta) @ np.linalg.inv(np.asarray(Tb))
    T1 = moved(np.asarray(Ta), xa) @ np.linalg.inv(moved(np.asarray(Tb), xb))
    return PC.pose_error(T0[:3, :3], T0[:3, 3], T1[:3, :3], T1[:3, 3])
