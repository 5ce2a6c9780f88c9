"""Inputs and recorded bounds of the rotated-view rectification tests (tests/test_rectify_views_ref.py on the CPU,
tests/test_gpu_rectify_views.py on the device).  The scene is one frame of a 640 x 480 equidistant fisheye (193 px/rad, a
193 degree lens whose rays are cut at 100 degrees from the axis) looking at six tags 45-70 units away at bearings from -78
to +75 degrees -- more than any single pinhole holds -- rectified into three 90 degree views at yaw -60, 0 and +60 degrees,
two tags per view.  The views overlap by 30 degrees so that no tag is cut by every view that sees it: the tag at -50 degrees
is cut by the front view's edge (-45) and whole in the left view, the one at -20 cut by the left view's edge (-15) and
whole in the front view.

Every bound below was measured on the CPU with the oracle detector, the NumPy statement (tests/rectify_views_ref.py) and,
for the rig pose, tests/rig_ref.py -- never with the kernel -- and carries a factor of 2; test_rectify_views_ref.py measures
them again and requires the recorded figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import oracle_lib as O
import rectify_views_ref as VR
import rig_ref as RGR
from aprilslam_amd import _lib, synth
from aprilslam_amd.families import get_family
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rectify import ViewSet

W, H = 640, 480
K = np.array([[193.0, 0.0, 320.0], [0.0, 193.0, 240.0], [0.0, 0.0, 1.0]])
DIST = np.array([-0.01, 0.003, -0.0005, 0.00002])
CUT = np.radians(100.0)      # the image circle: rays further from the axis show the background
N_VIEWS, HFOV, STEP = 3, 90.0, 60.0
SIZE = (640, 480)
MAX_TAGS = 8
BACKGROUND = (128, 0, 128)   # synth.render_frame's
# (id, bearing deg, distance, height y, tilt about x deg, tilt about y deg)
TAGS = [(0, -78.0, 48.0, 2.0, 8.0, -12.0), (1, -50.0, 62.0, -4.0, -10.0, 9.0), (2, -20.0, 55.0, 3.0, 12.0, 14.0),
        (3, 12.0, 70.0, -3.0, -7.0, -11.0), (4, 44.0, 45.0, 4.0, 9.0, 10.0), (5, 75.0, 58.0, -2.0, -13.0, 7.0)]
ONE_VIEW_HFOV = 100.0        # the TagDetector(lens_model="fisheye") test: one view, R the identity


def recorded():
    """{name: (measured, bound = 2 x measured)}, the measurements rounded up to 4 significant digits.
    corner_px: the oracle's corners on the statement's views against the true projection of the tag's corner points into
      the view, the largest difference over all six tags.  The views upsample the source by 320 / 193 = 1.66, so a source
      pixel's worth of edge position is 1.66 view pixels; the factor 2 is the project's for the resampling phase.
    tag_trans_rel / tag_rot_rad: the oracle's PnP of those corners with the view's K_new, taken into the source camera's
      frame through R, against the ground truth: translation relative to the distance, rotation in radians.
    rig_trans / rig_rot_rad: tests/rig_ref.py on the three views' observations with the six true poses as the map, against
      the identity (the rig frame is the source camera, the world frame too): translation in scene units, rotation in radians.
    margin_trans / margin_rot_rad: the amount by which the rig pose's error exceeds that of the best single view's own
      localisation (localize_ref.py on that view's two tags, taken into the rig frame).
      Both are 0: the best single view (the left one, 0.045 units and 0.00051 rad off) is five times worse in translation
      than the rig, so the GPU test asks that no single view beats the rig pose at all."""
    measured = {"corner_px": 0.8646, "tag_trans_rel": 0.009961, "tag_rot_rad": 0.06900, "rig_trans": 0.009348, "rig_rot_rad": 0.0002171,
                "margin_trans": 0.0, "margin_rot_rad": 0.0}
    return {k: (v, 2 * v) for k, v in measured.items()}


def view_set(theta_max=None):
    return ViewSet.fan(K, DIST, "fisheye", N_VIEWS, HFOV, SIZE, step_deg=STEP, theta_max=theta_max)


def one_view_K():
    f = 0.5 * W / np.tan(np.radians(0.5 * ONE_VIEW_HFOV))
    return np.array([[f, 0.0, 0.5 * W], [0.0, f, 0.5 * H], [0.0, 0.0, 1.0]])


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) if axis == "y" else np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


@functools.lru_cache(maxsize=None)
def ground_truth():
    """{id: source camera <- tag 4x4}: every tag faces the camera but for its two tilts"""
    gt = {}
    for i, bearing, dist, y, tx, ty in TAGS:
        T = np.eye(4)
        T[:3, :3] = _rot("y", bearing) @ _rot("x", tx) @ _rot("y", ty) @ np.diag([1.0, -1.0, -1.0])
        T[:3, 3] = [dist * np.sin(np.radians(bearing)), y, dist * np.cos(np.radians(bearing))]
        gt[i] = T
    return gt


def tag_map():
    """the six true poses, the world being the source camera's frame: the true pose world<-rig is the identity"""
    return TagMap.from_dict(ground_truth())


@functools.lru_cache(maxsize=None)
def fisheye_frame():
    """the (H, W, 3) BGR frame the fisheye delivers: per pixel the ray (fisheye_unproject), cut at CUT, against each tag's
    plane, far to near, the family texture sampled with synth._bilinear as synth.render_frame does"""
    fam = get_family()
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = VR.fisheye_unproject(xs, ys, K, DIST)
    seen = np.arccos(np.clip(d[..., 2], -1.0, 1.0)) <= CUT
    frame = np.empty((H, W, 3), dtype=np.uint8)
    frame[:] = BACKGROUND
    half = 0.5 * LC.TAG_OUTER
    gt = ground_truth()
    for i in sorted(gt, key=lambda i: -np.linalg.norm(gt[i][:3, 3])):
        R, t = gt[i][:3, :3], gt[i][:3, 3]
        with np.errstate(all="ignore"):
            s = (R[:, 2] @ t) / (d @ R[:, 2])          # the ray s d meets the tag's plane
        q = (s[..., None] * d - t) @ R                 # in the tag's frame
        inside = seen & (s > 0) & (np.abs(q[..., 0]) <= half) & (np.abs(q[..., 1]) <= half)
        tex = fam.texture(i, 40)
        th, tw = tex.shape[:2]
        u = (q[..., 0] + half) / (2 * half) * tw
        v = (1.0 - (q[..., 1] + half) / (2 * half)) * th
        rgb = synth._bilinear(tex, u[inside], v[inside])
        frame[inside] = np.clip(np.floor(rgb[:, ::-1] + 0.5), 0, 255).astype(np.uint8)
    frame.setflags(write=False)
    return frame


def true_corners(view_K, view_R, T):
    """the tag's four corner points (the PnP's, LC.TAG_INNER apart) projected into the view (K_new, R): (4, 2)"""
    obj = np.c_[LR.object_corners(LC.TAG_INNER), np.zeros(4)]
    P = (obj @ T[:3, :3].T + T[:3, 3]) @ view_R      # rows (R^T p)^T
    return np.stack([view_K[0, 0] * P[:, 0] / P[:, 2] + view_K[0, 2], view_K[1, 1] * P[:, 1] / P[:, 2] + view_K[1, 2]], axis=-1)


def in_source(view_R, T_view_tag):
    """view <- tag -> source camera <- tag"""
    E = np.eye(4)
    E[:3, :3] = view_R
    return E @ T_view_tag


def trans_err(T, T_ref):
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]) / np.linalg.norm(T_ref[:3, 3]))


def rot_err(T, T_ref):
    c = 0.5 * (np.trace(T[:3, :3].T @ T_ref[:3, :3]) - 1.0)
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def pose_errors(T):
    """(translation in scene units, rotation in radians) of a pose world<-rig against the identity"""
    return float(np.linalg.norm(T[:3, 3])), rot_err(T, np.eye(4))


def obs_rows(ids, corners, T, max_tags=MAX_TAGS):
    """one view's asl_obs row of one frame from detections (ids, (n, 4, 2) corners) and their PnP poses (n, 4, 4)"""
    row = np.zeros(max_tags, dtype=_lib.OBS_DTYPE)
    row["id"] = -1
    for k, (i, c, Tk) in enumerate(zip(ids, corners, T)):
        row["id"][k], row["flags"][k] = i, 3
        row["corners"][k] = np.asarray(c).ravel()
        row["T"][k] = np.asarray(Tk).ravel()[:12]
    return row


def single_view_errors(vs, obs, localize_one):
    """per view with a pose: the (translation, rotation) error of the view's own localisation, taken into the rig frame.
    localize_one(view index, (1, max_tags) obs, K_new) -> (1,) CAM_POSE_DTYPE world<-view"""
    out = []
    cams = vs.rig().cameras
    for v, (Kn, _) in enumerate(vs.views):
        p = localize_one(v, obs[v], Kn)[0]
        if p["status"] == 0:
            out.append(pose_errors(p["T"] @ cams[v].T_cam_rig))
    return out


@functools.lru_cache(maxsize=None)
def measure():
    """the seven figures of recorded(), measured now: oracle + statements only"""
    fam = get_family()
    vs = view_set()
    gt = ground_truth()
    views = VR.rectify_views(fisheye_frame(), K, DIST, VR.LENS_FISHEYE, vs.views, SIZE[0], SIZE[1])
    out = dict(corner_px=0.0, tag_trans_rel=0.0, tag_rot_rad=0.0)
    obs = np.zeros((len(vs), 1, MAX_TAGS), dtype=_lib.OBS_DTYPE)
    found = []
    for v, (Kn, R) in enumerate(vs.views):
        dets = O.detect_gray(views[v], fam)
        assert all(d["hamming"] == 0 for d in dets), v
        found += [(v, int(d["id"])) for d in dets]
        corners = np.stack([d["corners"] for d in dets])
        _, _, T, ok = O.solve_pnp(corners, Kn, np.zeros(0), LC.TAG_INNER)
        assert ok.all()
        for d, Tk in zip(dets, T):
            ref = gt[int(d["id"])]
            out["corner_px"] = max(out["corner_px"], float(np.abs(d["corners"] - true_corners(Kn, R, ref)).max()))
            out["tag_trans_rel"] = max(out["tag_trans_rel"], trans_err(in_source(R, Tk), ref))
            out["tag_rot_rad"] = max(out["tag_rot_rad"], rot_err(in_source(R, Tk), ref))
        obs[v, 0] = obs_rows([d["id"] for d in dets], corners, T)
    assert found == [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)], found
    rec = tag_map().as_records()
    pose = RGR.localize(obs, rec, vs.rig(), LC.TAG_INNER)[0]
    assert pose["status"] == 0
    out["rig_trans"], out["rig_rot_rad"] = pose_errors(pose["T"])
    single = single_view_errors(vs, obs, lambda v, o, Kn: LR.localize(o, rec, Kn, None, LC.TAG_INNER))
    assert len(single) == len(vs)
    out["margin_trans"] = max(0.0, out["rig_trans"] - min(e[0] for e in single))
    out["margin_rot_rad"] = max(0.0, out["rig_rot_rad"] - min(e[1] for e in single))
    out["single"] = single
    return out
