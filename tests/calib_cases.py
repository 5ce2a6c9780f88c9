"""Inputs of the calibration tests (tests/test_calib_ref.py on the CPU, tests/test_gpu_calibrate.py on the device): asl_obs
blocks from exact projections through a known camera, the planar board, the distorted webcam, and the error measures."""
import numpy as np

import calib_ref as CR
import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import synth
from aprilslam_amd.localize import TagMap

W, H = LC.W, LC.H
K_TRUE = np.array([[905.0, 0.0, 652.5], [0.0, 884.0, 347.0], [0.0, 0.0, 1.0]])   # fx != fy, principal point off the centre
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
DIST4 = DIST5[:4]
WEBCAM_W, WEBCAM_H, WEBCAM_FOV = 640, 480, 60.0
WEBCAM_DIST = np.array([-0.12, 0.05, 0.002, -0.0015, -0.01])   # test_gpu_render.py's mild wide-angle webcam
BOARD_ROWS, BOARD_COLS, BOARD_SPACING = 5, 7, 16.0


def board_scene(rows=BOARD_ROWS, cols=BOARD_COLS, spacing=BOARD_SPACING):
    """TagMap.grid's board as a synth scene (tags in the world's z = 0 plane, facing +z)"""
    return [{"id": r * cols + c, "position": [c * spacing, r * spacing, 0.0], "rotation": [0.0, 0.0, 0.0]}
            for r in range(rows) for c in range(cols)]


def board_cameras(n, fronto=False, seed=7):
    """cameras in front of the board (synth's camera looks down -z): tilted views, or fronto-parallel ones"""
    rng = np.random.default_rng(seed)
    cx, cy = 0.5 * (BOARD_COLS - 1) * BOARD_SPACING, 0.5 * (BOARD_ROWS - 1) * BOARD_SPACING
    out = []
    for _ in range(n):
        if fronto:
            out.append(((cx + rng.uniform(-15, 15), cy + rng.uniform(-10, 10), rng.uniform(170, 230)), (0.0, 0.0, 0.0)))
        else:
            pitch, yaw = rng.uniform(-25, 25), rng.uniform(-25, 25)
            d = rng.uniform(110, 140)
            # look at the board centre from a tilted direction: pull the camera back along its own view axis
            R = synth._ry(np.radians(yaw)) @ synth._rx(np.radians(pitch))
            pos = np.array([cx, cy, 0.0]) + R @ np.array([0.0, 0.0, d])
            out.append((tuple(pos), (pitch, yaw, rng.uniform(-10, 10))))
    return out


def exact_block(tags, cams, K, dist, max_tags=24, width=W, height=H):
    return np.stack([LC.exact_frame(tags, p, r, K, dist=dist, max_tags=max_tags, width=width, height=height) for p, r in cams])


def scene_case(K=K_TRUE, dist=DIST5, n=16):
    """the bench scene (20 tags, not planar) from the bench trajectory, exact corners"""
    tags = LC.bench_scene()
    cams = LC.trajectory(n)
    return exact_block(tags, cams, K, dist), TagMap.from_scene(tags).as_records(), [LC.world_from_camera(p, r) for p, r in cams]


def board_case(K=K_TRUE, dist=DIST5, n=12, fronto=False):
    """TagMap.grid's board, exact corners"""
    tags = board_scene()
    cams = board_cameras(n, fronto)
    rec = TagMap.grid(BOARD_ROWS, BOARD_COLS, LC.TAG_INNER, BOARD_SPACING).as_records()
    return exact_block(tags, cams, K, dist, max_tags=40), rec, [LC.world_from_camera(p, r) for p, r in cams]


def distortion_field(K, dist, width, height, n=16):
    """pixel displacement the lens adds at an n x n grid over the image (each model with its own K), (n * n, 2)"""
    K = np.asarray(K, dtype=np.float64)
    u, v = np.meshgrid(np.linspace(0, width, n), np.linspace(0, height, n))
    x, y = (u.ravel() - K[0, 2]) / K[0, 0], (v.ravel() - K[1, 2]) / K[1, 1]
    P = np.stack([x, y, np.ones_like(x)], axis=1)
    return LR.project(LR.camera(K, dist), P) - LR.project(LR.camera(K, None), P)


def field_err(res_K, res_dist, K, dist, width=W, height=H):
    return float(np.abs(distortion_field(res_K, res_dist, width, height) - distortion_field(K, dist, width, height)).max())


def cpu_cases():
    """(name, obs, map records, kwargs of calibrate) of the statement tests, for the kernel comparison"""
    sc, rec, _ = scene_case()
    bd, brec, _ = board_case(dist=DIST4)
    out = [("scene5", sc, rec, dict(n_dist=5)),
           ("board4", bd, brec, dict(n_dist=4)),
           ("scene0", scene_case(dist=None)[0], rec, dict(n_dist=0)),
           ("fix_pp", sc, rec, dict(n_dist=5, flags=CR.FIX_PRINCIPAL_POINT, K_init=K_TRUE + np.diag([5.0, -4.0, 0.0]))),
           ("fix_aspect", sc, rec, dict(n_dist=5, flags=CR.FIX_ASPECT_RATIO)),
           ("zero_tangent", bd, brec, dict(n_dist=4, flags=CR.ZERO_TANGENT_DIST, max_iters=12)),
           ("fronto", board_case(n=6, fronto=True)[0], brec, dict(n_dist=5))]
    padded = np.zeros((sc.shape[0] + 3, sc.shape[1]), dtype=sc.dtype)
    padded["id"] = -1
    padded[[0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 17, 18]] = sc
    padded["id"][8, 0], padded["flags"][8, 0] = 999, 1      # an unmapped id only
    out.append(("padded", padded, rec, dict(n_dist=5)))
    one = sc[:1].copy()
    one["flags"][0, 1:] = 0
    out.append(("one_tag", one, rec, dict(n_dist=5)))
    return out
