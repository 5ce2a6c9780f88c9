"""Inputs and recorded bounds of the fisheye calibration tests (tests/test_calib_fisheye_ref.py on the CPU,
tests/test_gpu_calibrate_fisheye.py on the device): asl_obs blocks of TagMap.grid's 5 x 7 board seen through a 640 x 480
fisheye of about 193 px/rad (fx != fy, the principal point a few pixels off the centre, rectify_views_cases' coefficients),
corners projected exactly and rounded to float32 as the records hold them; the error measures; and the end-to-end scene,
host-ray-traced fisheye frames of a 3 x 4 board.

A view: the camera faces the board's centre from 35-70 units with tilts within +-30 degrees, and is then turned about an
axis across its own so that the board's centre sits up to about 55 degrees off axis; a tag is in view if all its corners
land inside the image.

Every recorded bound was measured on the CPU with the NumPy statement (tests/calib_fisheye_ref.py) and, for the end-to-end
scene, the oracle detector -- never with the kernel -- and carries the project's factor of 2; test_calib_fisheye_ref.py
measures them again and requires the recorded figures to still hold."""
import functools

import numpy as np

import calib_fisheye_ref as FR
import localize_cases as LC
import localize_ref as LR
import rectify_views_cases as VC
import rectify_views_ref as VR
from aprilslam_amd import _lib, rectify, synth
from aprilslam_amd.families import get_family
from aprilslam_amd.localize import TagMap

W, H = 640, 480
K_TRUE = np.array([[193.0, 0.0, 323.5], [0.0, 191.0, 237.0], [0.0, 0.0, 1.0]])
DIST = VC.DIST
ROWS, COLS, SPACING = 5, 7, 16.0
MAX_TAGS = 40
R0 = np.diag([1.0, -1.0, -1.0])          # the board faces the camera: its z axis points at it
NOISE_PX, NOISE_SEED = 0.3, 5
# (distance, tilt about x deg, tilt about y deg, roll deg, turn deg, direction of the turn in the image plane deg)
VIEWS = [(38.0, 12.0, -20.0, 5.0, 55.0, 0.0), (45.0, -25.0, 15.0, -8.0, 50.0, 180.0), (60.0, 20.0, 28.0, 12.0, 35.0, 90.0),
         (70.0, -15.0, -28.0, -4.0, 30.0, 250.0), (35.0, 28.0, 8.0, 170.0, 52.0, 20.0), (52.0, -8.0, -12.0, 85.0, 5.0, 300.0)]
# the end-to-end scene: a 3 x 4 board of ids 0..11, 26 units between centres
E2E_ROWS, E2E_COLS, E2E_SPACING = 3, 4, 26.0
E2E_VIEWS = [(70.0, 10.0, -18.0, 4.0, 35.0, 0.0), (80.0, -22.0, 12.0, -6.0, 30.0, 180.0), (90.0, 18.0, 24.0, 10.0, 20.0, 90.0),
             (75.0, -14.0, -24.0, -3.0, 25.0, 270.0), (65.0, 24.0, 6.0, 175.0, 38.0, 15.0), (85.0, -6.0, -10.0, 88.0, 5.0, 300.0)]


def recorded():
    """{name: (measured, bound = 2 x measured)}, the measurements rounded up to 4 significant digits.
    noisy_*: `board4`'s corners with NOISE_PX of Gaussian noise (seed NOISE_SEED) through the statement: the larger relative
      error of fx and fy, the larger error of cx and cy in pixels, and the distortion-field error (field_err) in pixels.
    e2e_*: the same three of the end-to-end scene: the oracle detector's corners on the ray-traced frames through the
      statement."""
    measured = {"noisy_f_rel": MEASURED_NOISY[0], "noisy_c_px": MEASURED_NOISY[1], "noisy_field_px": MEASURED_NOISY[2],
                "e2e_f_rel": MEASURED_E2E[0], "e2e_c_px": MEASURED_E2E[1], "e2e_field_px": MEASURED_E2E[2]}
    return {k: (v, 2 * v) for k, v in measured.items()}


MEASURED_NOISY = (0.0002240, 0.07472, 0.2033)
MEASURED_E2E = (0.003651, 0.2600, 1.098)


def _rx(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _ry(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def board_map(rows=ROWS, cols=COLS, spacing=SPACING):
    return TagMap.grid(rows, cols, LC.TAG_INNER, spacing)


def view_pose(view, rows=ROWS, cols=COLS, spacing=SPACING):
    """camera<-world (R, t) of one view of the board"""
    d, tx, ty, roll, turn, direction = view
    centre = np.array([0.5 * (cols - 1) * spacing, 0.5 * (rows - 1) * spacing, 0.0])
    Rf = _rz(roll) @ _rx(tx) @ _ry(ty) @ R0                # facing the board's centre, d away
    tf = np.array([0.0, 0.0, d]) - Rf @ centre
    Rt = _rz(direction) @ _ry(-turn) @ _rz(-direction)     # the camera turns: the centre moves `turn` off axis, towards `direction`
    return Rt @ Rf, Rt @ tf


def world_from_camera(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
    return T


def exact_row(rec, R, t, K, dist, max_tags=MAX_TAGS, noise=None):
    """one frame's asl_obs row: every tag of the map records whose four corners project inside the image, in id order;
    noise: an optional (rng, sigma px) added to the corners before the rounding to float32"""
    cam = FR.camera(K, dist)
    row = np.zeros(max_tags, dtype=_lib.OBS_DTYPE)
    row["id"] = -1
    k = 0
    for i in range(len(rec)):
        h = LR.tag_half(rec[i], LC.TAG_INNER)[0]
        if h is None:
            continue
        P = LR._world_corners(rec["T"][i], LR.half_corners(h)) @ R.T + t
        uv = FR.project(cam, P)
        if np.any(uv < 0) or np.any(uv[:, 0] >= W) or np.any(uv[:, 1] >= H):
            continue
        if noise is not None:
            uv = uv + noise[0].normal(0.0, noise[1], uv.shape)
        row["id"][k], row["flags"][k] = i, 1
        row["corners"][k] = uv.ravel()
        k += 1
    return row


@functools.lru_cache(maxsize=None)
def board_block(with_k=True, noisy=False):
    """(obs (6, MAX_TAGS), map records, [camera<-world (R, t)]) of VIEWS; with_k False: the pure equidistant lens"""
    rec = board_map().as_records()
    poses = [view_pose(v) for v in VIEWS]
    rng = np.random.default_rng(NOISE_SEED)
    obs = np.stack([exact_row(rec, R, t, K_TRUE, DIST if with_k else None, noise=(rng, NOISE_PX) if noisy else None) for R, t in poses])
    obs.setflags(write=False)
    return obs, rec, poses


def off_axis_deg(obs, rec, poses):
    """the angle off axis of every used corner of every frame, from the true poses: a flat array in degrees"""
    out = []
    for row, (R, t) in zip(obs, poses):
        for o in row[row["flags"] & 1 == 1]:
            P = LR._world_corners(rec["T"][o["id"]], LR.half_corners(LR.tag_half(rec[o["id"]], LC.TAG_INNER)[0])) @ R.T + t
            out.append(np.degrees(np.arctan2(np.hypot(P[:, 0], P[:, 1]), P[:, 2])))
    return np.concatenate(out)


def on_axis_frame(rec):
    """a frame whose camera looks straight at the lb corner of tag 17 from 40 units: that corner's camera point is exactly
    (0, 0, 40) -- R0 and the translation are exact in float64 -- and its pixel exactly (cx, cy)"""
    h = LR.tag_half(rec[17], LC.TAG_INNER)[0]
    c = rec["T"][17].reshape(3, 4) @ np.array([-h, -h, 0.0, 1.0])
    t = np.array([-c[0], c[1], 40.0])
    return R0.copy(), t


def far_only_frame(rec):
    """a frame that keeps only tags with a corner more than 1.3 rad off the axis of K_INIT_NEAR: of view 0, turned 55 degrees"""
    R, t = view_pose(VIEWS[0])
    row = exact_row(rec, R, t, K_TRUE, DIST)
    Kn = K_INIT_NEAR
    for k in range(len(row)):
        if row["flags"][k] and FR.slot_rays(row["corners"][k], Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2])[0]:
            row["flags"][k], row["id"][k] = 0, -1
    return row


K_INIT_NEAR = K_TRUE + np.array([[4.0, 0.0, 5.0], [0.0, -3.0, -4.0], [0.0, 0.0, 0.0]])
K_INIT_HALF_W = np.array([[0.5 * W, 0.0, 0.5 * W], [0.0, 0.5 * W, 0.5 * H], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, obs, map records, kwargs of calibrate)]"""
    b4, rec, _ = board_block()
    b0, _, _ = board_block(with_k=False)
    out = [("board4", b4, rec, dict(n_dist=4)),
           ("board0", b0, rec, dict(n_dist=0)),
           ("fix_pp", b4, rec, dict(n_dist=4, flags=FR.FIX_PRINCIPAL_POINT, K_init=K_INIT_NEAR)),
           ("fix_aspect", b4, rec, dict(n_dist=4, flags=FR.FIX_ASPECT_RATIO)),
           ("k_init", b4, rec, dict(n_dist=4, K_init=K_INIT_HALF_W))]
    padded = np.zeros((b4.shape[0] + 3, b4.shape[1]), dtype=b4.dtype)
    padded["id"] = -1
    padded[[0, 2, 3, 5, 6, 8]] = b4
    padded["id"][4, 0], padded["flags"][4, 0] = 999, 1      # an unmapped id only
    out.append(("padded", padded, rec, dict(n_dist=4)))
    one = b4[:1].copy()
    one["flags"][0, 1:] = 0
    out.append(("one_tag", one, rec, dict(n_dist=4)))
    Ra, ta = on_axis_frame(rec)
    out.append(("on_axis", np.concatenate([b4, exact_row(rec, Ra, ta, K_TRUE, DIST)[None]]), rec, dict(n_dist=4)))
    # K_init: under the ladder such a frame has candidates at the wide rungs only and would move the choice of rung
    out.append(("far_only", np.concatenate([b4[:3], far_only_frame(rec)[None], b4[3:]]), rec, dict(n_dist=4, K_init=K_INIT_NEAR)))
    return out


def case(name):
    return [c for c in cases() if c[0] == name][0]


def field_err(K_a, dist_a, K_b, dist_b, n=16, max_deg=95.0):
    """the largest pixel difference of the two lenses, each with its own K, over an n x n grid of rays within max_deg of
    the axis (rectify.project_rays)"""
    a = np.radians(np.linspace(-max_deg, max_deg, n))
    ax, ay = np.meshgrid(a, a)
    th = np.hypot(ax, ay)
    keep = th <= np.radians(max_deg)
    with np.errstate(all="ignore"):
        k = np.where(th > 0, np.sin(th) / th, 1.0)
    rays = np.stack([k * ax, k * ay, np.cos(th)], axis=-1)[keep]
    pa = rectify.project_rays(rays, K_a, dist_a, "fisheye")
    pb = rectify.project_rays(rays, K_b, dist_b, "fisheye")
    return float(np.abs(pa - pb).max())


def lens_errors(res, K=K_TRUE, dist=DIST):
    """(the larger relative error of fx and fy, the larger error of cx and cy in pixels, field_err) of a result record"""
    Kr = res["K"]
    f = max(abs(Kr[0, 0] / K[0, 0] - 1), abs(Kr[1, 1] / K[1, 1] - 1))
    c = max(abs(Kr[0, 2] - K[0, 2]), abs(Kr[1, 2] - K[1, 2]))
    return float(f), float(c), field_err(Kr, res["dist"][:4], K, np.zeros(4) if dist is None else dist)


def measure_noisy():
    obs, rec, _ = board_block(noisy=True)
    res, _ = FR.calibrate(obs, rec, LC.TAG_INNER, W, H, n_dist=4)
    assert res["status"] == 0
    return lens_errors(res)


# ---- the end-to-end scene: ray-traced fisheye frames

def e2e_map():
    return board_map(E2E_ROWS, E2E_COLS, E2E_SPACING)


def e2e_poses():
    return [view_pose(v, E2E_ROWS, E2E_COLS, E2E_SPACING) for v in E2E_VIEWS]


def fisheye_frame(tag_T, K, dist, cut=VC.CUT):
    """rectify_views_cases.fisheye_frame for any set of tags: tag_T {id: camera<-tag 4x4} -> the (H, W, 3) BGR frame the
    fisheye delivers: per pixel the ray (fisheye_unproject), cut at `cut`, against each tag's plane, far to near, the
    family texture sampled with synth._bilinear as synth.render_frame does"""
    fam = get_family()
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = VR.fisheye_unproject(xs, ys, K, dist)
    seen = np.arccos(np.clip(d[..., 2], -1.0, 1.0)) <= cut
    frame = np.empty((H, W, 3), dtype=np.uint8)
    frame[:] = VC.BACKGROUND
    half = 0.5 * LC.TAG_OUTER
    for i in sorted(tag_T, key=lambda i: -np.linalg.norm(tag_T[i][:3, 3])):
        R, t = tag_T[i][:3, :3], tag_T[i][:3, 3]
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
    return frame


@functools.lru_cache(maxsize=None)
def e2e_frames():
    """(6, H, W, 3) uint8: the board of e2e_map from e2e_poses through the true lens"""
    tm = e2e_map()
    out = []
    for R, t in e2e_poses():
        Tcw = np.eye(4)
        Tcw[:3, :3], Tcw[:3, 3] = R, t
        out.append(fisheye_frame({i: Tcw @ T for i, T in tm.poses.items()}, K_TRUE, DIST))
    frames = np.stack(out)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def e2e_oracle_obs():
    """the oracle detector's hamming-0 detections of the board's ids on e2e_frames as an asl_obs block (6, 12)"""
    import oracle_lib as O
    fam = get_family()
    n_ids = E2E_ROWS * E2E_COLS
    obs = np.zeros((len(E2E_VIEWS), n_ids), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    for f, frame in enumerate(e2e_frames()):
        dets = [d for d in O.detect_bgr(np.ascontiguousarray(frame), fam) if d["hamming"] == 0 and d["id"] < n_ids]
        for k, d in enumerate(sorted(dets, key=lambda d: d["id"])):
            obs["id"][f, k], obs["flags"][f, k] = d["id"], 1
            obs["corners"][f, k] = np.asarray(d["corners"], dtype=np.float32).ravel()
    return obs


def measure_e2e():
    """(lens_errors of the statement on the oracle's corners, the statement's result and poses, the block)"""
    obs = e2e_oracle_obs()
    res, poses = FR.calibrate(obs, e2e_map().as_records(), LC.TAG_INNER, W, H, n_dist=4)
    assert res["status"] == 0
    return lens_errors(res), res, poses, obs
