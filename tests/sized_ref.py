"""NumPy statement of the solvers that take a tag map whose entries carry their own size (asl_map_tag.size): localisation
of one camera and of a rig with their covariance forms, calibration and the sequence solves.  Test infrastructure.

The rule (map_tag_half, aprilslam_amd/csrc/k_localize.inc):

  size == 0            the tag has the call's tag_size: half = float32(tag_size / 2), as before
  size > 0, finite     the tag's own side: half = float32(size) * float32(0.5) (halving a float32 is exact)
  negative, not finite the entry counts as valid = 0

and where it enters:

  gather   a slot's world corners are (+-half, +-half, 0) of ITS tag through the map pose (localize_ref.frame_points,
           calib_ref.gather); an entry with a bad size is an unmapped id (localize_ref.gather).  Every pass after the
           gather reads these points, so the refinement, the gate, the Huber passes, the covariances and the sequence
           solve's linearisation need no statement of their own.
  seed     a record's PnP pose T was solved at the call's tag_size.  For a tag of half h_id it has the right rotation and
           a translation short by half / h_id: scaling the object and the translation together leaves every ray where it
           is, under any lens.  A sized slot's candidates (plain and mirrored) are built from T with its translation
           times k = h_id / half; a slot without a size takes the unscaled path (localize_ref.seed_candidates).
           The calibration forms its planar pose at the slot's own half (calib_ref.seed_frame).  Candidate B of the
           sequence solve comes from the map pose and the seed pose, not from a PnP pose: unchanged.

The existing statements fix one tag_size inside exactly these functions and call them by their module names, so this file
restates those functions (gather, frame_points, seed_candidates; calib_ref's gather and seed_frame) and runs the existing
statements with them in place (honoured): every other line of localize_ref, rig_ref, pose_cov_ref, calib_ref and the
smooth_* family is the one already there.  With every size 0 the restated functions do the same arithmetic in the same
order, so the results are the existing statements' byte for byte (tests/test_sized_ref.py).
"""
import contextlib
import functools

import numpy as np

import calib_ref as CR
import localize_ref as LR
import rig_ref as RR
import smooth_cov_ref as SV
import smooth_ref as SR


def tag_half(tag_map, tag_id, tag_size):
    """(half side of map entry tag_id, whether it is the tag's own), or (None, False) for an entry that does not take part"""
    e = tag_map[tag_id]
    size = np.float32(e["size"])
    if not e["valid"] or not (np.isfinite(size) and size >= 0):
        return None, False
    if size > 0:
        return float(size * np.float32(0.5)), True
    return LR.half_size(tag_size), False


def tag_pose(tag_map, tag_id, T_cam_tag, tag_size):
    """camera<-tag (3x4) of a sized tag from the pose the per-tag PnP gave at tag_size: translation times k"""
    T = np.array(T_cam_tag, dtype=np.float64).reshape(-1, 4)[:3].copy()
    h, own = tag_half(tag_map, tag_id, tag_size)
    if own:
        T[:, 3] = T[:, 3] * (h / LR.half_size(tag_size))
    return T


def _object_corners(h):
    return np.array([[-h, -h], [h, -h], [h, h], [-h, h]], dtype=np.float64)


def gather(rows, tag_map):
    """localize_ref.gather with the validity rule of tag_half"""
    flat = rows.reshape(-1)
    n_ids = len(tag_map)
    part = [s for s, o in enumerate(flat) if (o["flags"] & 1) and 0 <= o["id"] < n_ids and tag_half(tag_map, o["id"], 1.0)[0] is not None]
    seeds = [s for s in part if flat["flags"][s] & 2]
    return flat, part, seeds


def frame_points(model, rows, tag_map, tag_size, slots):
    """localize_ref.frame_points with every slot's own half"""
    flat = rows.reshape(-1)
    Xw = np.concatenate([LR._world_corners(tag_map["T"][flat["id"][s]], _object_corners(tag_half(tag_map, flat["id"][s], tag_size)[0]))
                         for s in slots])
    uv = np.concatenate([flat["corners"][s].astype(np.float64).reshape(4, 2) for s in slots])
    ci = np.repeat(np.array([model.slot_camera(s, rows.shape[-1]) for s in slots], dtype=np.int64), 4)
    return Xw, uv, ci


def seed_candidates(model, rows, tag_map, seeds, Xw, uv, ci, tag_size):
    """localize_ref.seed_candidates; a sized slot's PnP translation times k = h_id / half before the mirrored minimum"""
    flat = rows.reshape(-1)
    chosen = [seeds[k] for k in LR.top_k([LR.corner_area(flat["corners"][s]) for s in seeds])]
    half = LR.half_size(tag_size)
    out = []
    for s in chosen:
        To = flat["T"][s].reshape(3, 4)
        M = tag_map["T"][flat["id"][s]].reshape(3, 4)
        h, own = tag_half(tag_map, flat["id"][s], tag_size)
        to0 = To[:, 3] * (h / half) if own else To[:, 3]
        for m in (0, 1):
            Ro, to = To[:, :3], to0
            if m:
                Ro, to = LR.mirrored(Ro, to)
            Rk = Ro @ M[:, :3].T                    # camera<-world = T_obs inv(map)
            tk = to - Rk @ M[:, 3]
            Rc, tc = model.pose(Rk, tk, model.slot_camera(s, rows.shape[-1]))
            out.append((Rc, tc, s + LR.MIRRORED * m, float(model.costs(Rc, tc, Xw, uv, ci).sum())))
    return chosen, out


def calib_gather(rows, tag_map, tag_size):
    """calib_ref.gather with the validity rule and every slot's own half"""
    n_ids = len(tag_map)
    part = [s for s, o in enumerate(rows) if (o["flags"] & 1) and 0 <= o["id"] < n_ids and tag_half(tag_map, o["id"], tag_size)[0] is not None]
    if not part:
        return part, np.zeros((0, 3)), np.zeros((0, 2))
    Xw = np.concatenate([LR._world_corners(tag_map["T"][rows["id"][s]], _object_corners(tag_half(tag_map, rows["id"][s], tag_size)[0]))
                         for s in part])
    uv = np.concatenate([rows["corners"][s].astype(np.float64).reshape(4, 2) for s in part])
    return part, Xw, uv


def calib_seed_frame(rows, part, Xw, uv, tag_map, theta0, width, height, tag_size):
    """calib_ref.seed_frame with the planar pose of every slot at its own half"""
    fx, fy, cx, cy = theta0[:4]
    cam0 = (fx, fy, cx, cy, 0.0, 0.0, 0.0, 0.0, 0.0)
    s = 0.5 * (width + height)
    best, best_cost = None, np.inf
    for k in [part[i] for i in LR.top_k([LR.corner_area(rows["corners"][k]) for k in part])]:
        half = tag_half(tag_map, rows["id"][k], tag_size)[0]
        Ro, to = CR.planar_pose(CR.square_homography(rows["corners"][k], cx, cy, s), fx, fy, s, half)
        M = tag_map["T"][rows["id"][k]].reshape(3, 4)
        for m in (0, 1):
            Rk, tk = LR.mirrored(Ro, to) if m else (Ro, to)
            Rc = Rk @ M[:, :3].T
            tc = tk - Rc @ M[:, 3]
            c = float(LR.corner_costs(cam0, Rc, tc, Xw, uv).sum())
            if c < best_cost:
                best, best_cost = (Rc, tc, k + LR.MIRRORED * m), c
    if best is None or not best_cost < LR.BEHIND_COST:
        return None
    R, t, cost = LR.lm(LR.corner_lin(cam0, Xw, uv), best[0], best[1])
    return R, t, cost, best[2]


@contextlib.contextmanager
def honoured(tag_size):
    """the existing statements with the functions above where theirs fix one tag_size; theirs come back on leaving"""
    swaps = [(LR, "gather", gather), (LR, "frame_points", frame_points),
             (LR, "seed_candidates", functools.partial(seed_candidates, tag_size=tag_size)),
             (CR, "gather", calib_gather), (CR, "seed_frame", calib_seed_frame)]
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in swaps]
    try:
        for mod, name, fn in swaps:
            setattr(mod, name, fn)
        yield
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)


def localize(obs, tag_map, K, dist, tag_size, max_tag_rms_px=0.0, sigma_px=None, traces=None):
    """localize_ref.localize over a sized map"""
    with honoured(tag_size):
        return LR.localize(obs, tag_map, K, dist, tag_size, max_tag_rms_px, sigma_px, traces)


def localize_rig(obs, tag_map, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None, traces=None):
    """rig_ref.localize over a sized map"""
    with honoured(tag_size):
        return RR.localize(obs, tag_map, rig, tag_size, max_tag_rms_px, sigma_px, traces)


def calibrate(obs, tag_map, tag_size, width, height, **kw):
    """calib_ref.calibrate over a sized map"""
    with honoured(tag_size):
        return CR.calibrate(obs, tag_map, tag_size, width, height, **kw)


def smooth(obs, tag_map, K, dist, tag_size, seed, times, *args, **kw):
    """smooth_ref.smooth over a sized map"""
    with honoured(tag_size):
        return SR.smooth(obs, tag_map, K, dist, tag_size, seed, *args, times=times, **kw)


def smooth_cov(obs, tag_map, K, dist, tag_size, poses, result, times, *args, **kw):
    """smooth_cov_ref.smooth_cov over a sized map"""
    with honoured(tag_size):
        return SV.smooth_cov(obs, tag_map, K, dist, tag_size, poses, result, *args, times=times, **kw)


def smooth_rig(obs, tag_map, rig, tag_size, seed, *args, **kw):
    """smooth_ref.smooth_rig over a sized map"""
    with honoured(tag_size):
        return SR.smooth_rig(obs, tag_map, rig, tag_size, seed, *args, **kw)
