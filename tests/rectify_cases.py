"""Inputs and recorded bounds of the rectification tests (tests/test_rectify_ref.py on the CPU, tests/test_gpu_rectify.py on
the device).  Every bound below was measured on the CPU with the oracle detector and the NumPy statement
(tests/rectify_ref.py) -- never with the kernel -- and carries a factor of 2; test_rectify_ref.py measures them again and
requires the recorded figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import calib_cases as CC
import localize_cases as LC
import oracle_lib as O
import rectify_ref as RR
from aprilslam_amd import synth
from aprilslam_amd.families import get_family

W, H = CC.WEBCAM_W, CC.WEBCAM_H
N_TAGS = 6
# a barrel lens strong enough to bend a tag's edges, and the pinhole it is rectified to: a shorter focal length (wider
# field of view) keeps what the barrel pulled towards the centre in view
WIDE_FOV, WIDE_DIST, WIDE_FOV_NEW = 70.0, np.array([-0.30, 0.08, 0.0, 0.0, -0.008]), 80.0
# (name, fov of K, lens, fov of K_new, scene seed): the scenes of the comparison against the renderer's model
MODEL_SCENES = [("webcam%d" % s, CC.WEBCAM_FOV, CC.WEBCAM_DIST, CC.WEBCAM_FOV, s) for s in (1, 2, 3)] + \
               [("wide%d" % s, WIDE_FOV, WIDE_DIST, WIDE_FOV_NEW, s) for s in (1, 2, 3)]
WIDE_SCENE = MODEL_SCENES[3]

# The 8-frame mild-lens stream under CC.WEBCAM_DIST; the seed is one at which every tag stays in view of both paths (at
# the same K a barrel lens shows more of the scene than its rectified frame does, so a tag at the border can drop out).
MILD_SEED, MILD_FRAMES = 13, 8


def recorded():
    """{name: (measured, bound = 2 x measured)}, the measurements rounded up to 4 significant digits.
    model_corner_px: corners of the oracle on the statement-rectified lens render against its corners on the pinhole render
      of the same scene, the largest difference over MODEL_SCENES (rms 0.15 px, no bias).  Both frames sample the tag texture
      once per pixel centre; the rectified one is resampled bilinearly a second time, which moves an edge by a fraction of a
      pixel that depends on its phase against the grid: hence the factor 2 for scenes not looked at.
    wide_trans_rel / wide_rot_rad: those two frames of WIDE_SCENE through the oracle's PnP with K_new: the largest per-tag
      difference in translation (relative to the distance) and in rotation (radians).  The factor 2 for the same reason.
    mild_*: path A detects on the raw frames of the stream and solves with the lens (n_dist = 5), path B detects on the
      rectified frames and solves with the pinhole.  mild_corner_px: the largest distance between A's corners and B's
      corners taken through distort_points.  mild_trans_excess_rel / mild_rot_excess_rad: the largest amount by which B's
      per-tag pose error against the ground truth exceeds A's.  Factor 2: the same resampling phase, here moving with
      the camera from frame to frame."""
    measured = {"model_corner_px": 0.5608, "wide_trans_rel": 0.004526, "wide_rot_rad": 0.02258, "mild_corner_px": 0.4715,
                "mild_trans_excess_rel": 0.003442, "mild_rot_excess_rad": 0.008881}
    return {k: (v, 2 * v) for k, v in measured.items()}


def cameras(fov, fov_new):
    return synth.camera_matrix(W, H, fov), synth.camera_matrix(W, H, fov_new)


def scene_tags(fov_new, seed):
    return synth.random_scene(W, H, N_TAGS, np.random.default_rng(seed), fov_y_deg=fov_new)


@functools.lru_cache(maxsize=None)
def model_frames(name):
    """(pinhole render under K_new, lens render under K, the statement's rectification of it, ground truth, K, K_new, dist)"""
    _, fov, dist, fov_new, seed = [s for s in MODEL_SCENES if s[0] == name][0]
    tags = scene_tags(fov_new, seed)
    K, Kn = cameras(fov, fov_new)
    pin, gt = synth.render_frame(W, H, tags, LC.TAG_OUTER, fov_y_deg=fov_new)
    raw, _ = synth.render_frame(W, H, tags, LC.TAG_OUTER, fov_y_deg=fov, dist=dist)
    rect = RR.rectify(raw, K, dist, Kn, W, H)
    for a in (pin, raw, rect):
        a.setflags(write=False)
    return pin, raw, rect, gt, K, Kn, dist


def mild_stream():
    """(tags, cameras [(position, rotation_deg)]) of the 8-frame stream under CC.WEBCAM_DIST"""
    rng = np.random.default_rng(MILD_SEED)
    tags = synth.random_scene(W, H, N_TAGS, rng, fov_y_deg=CC.WEBCAM_FOV)
    return tags, [(tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-4, 4, 3))) for _ in range(MILD_FRAMES)]


def trans_err(T, T_ref):
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3]) / np.linalg.norm(T_ref[:3, 3]))


def rot_err(T, T_ref):
    c = 0.5 * (np.trace(T[:3, :3].T @ T_ref[:3, :3]) - 1.0)
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def oracle_poses(dets, K, dist):
    """{id: camera<-tag 4x4} of oracle detections through the oracle's PnP"""
    if not dets:
        return {}
    _, _, T, ok = O.solve_pnp(np.stack([d["corners"] for d in dets]), K, np.zeros(0) if dist is None else dist, LC.TAG_INNER)
    assert ok.all()
    return {int(d["id"]): T[i] for i, d in enumerate(dets)}


def pose_excess(pose_a, pose_b, gt):
    """largest amount by which pose_b's error against gt exceeds pose_a's, per tag: (translation, rotation), >= 0"""
    et = max([0.0] + [trans_err(pose_b[i], gt[i]) - trans_err(pose_a[i], gt[i]) for i in pose_a])
    er = max([0.0] + [rot_err(pose_b[i], gt[i]) - rot_err(pose_a[i], gt[i]) for i in pose_a])
    return et, er


@functools.lru_cache(maxsize=None)
def measure():
    """the six figures of recorded(), measured now: oracle + statement only"""
    fam = get_family()
    out = {"model_corner_px": 0.0}
    for name, *_ in MODEL_SCENES:
        pin, _, rect, gt, K, Kn, dist = model_frames(name)
        a, b = O.detect_bgr(pin, fam), O.detect_gray(rect, fam)
        assert [d["id"] for d in a] == [d["id"] for d in b] == sorted(gt), name
        out["model_corner_px"] = max([out["model_corner_px"]] + [float(np.abs(x["corners"] - y["corners"]).max()) for x, y in zip(a, b)])
        if name == WIDE_SCENE[0]:
            pa, pb = oracle_poses(a, Kn, None), oracle_poses(b, Kn, None)
            out["wide_trans_rel"] = max(trans_err(pb[i], pa[i]) for i in pa)
            out["wide_rot_rad"] = max(rot_err(pb[i], pa[i]) for i in pa)
    tags, cams = mild_stream()
    K = synth.camera_matrix(W, H, CC.WEBCAM_FOV)
    out.update(mild_corner_px=0.0, mild_trans_excess_rel=0.0, mild_rot_excess_rad=0.0)
    for pos, rot in cams:
        raw, gt = synth.render_frame(W, H, tags, LC.TAG_OUTER, cam_position=pos, cam_rotation_deg=rot, fov_y_deg=CC.WEBCAM_FOV,
                                     dist=CC.WEBCAM_DIST)
        rect = RR.rectify(raw, K, CC.WEBCAM_DIST, K, W, H)
        a, b = O.detect_bgr(raw, fam), O.detect_gray(rect, fam)
        assert [d["id"] for d in a] == [d["id"] for d in b], (pos, rot)
        for x, y in zip(a, b):
            back = RR.distort_points(y["corners"], K, CC.WEBCAM_DIST, K)
            out["mild_corner_px"] = max(out["mild_corner_px"], float(np.abs(back - x["corners"]).max()))
        et, er = pose_excess(oracle_poses(a, K, CC.WEBCAM_DIST), oracle_poses(b, K, None), gt)
        out["mild_trans_excess_rel"] = max(out["mild_trans_excess_rel"], et)
        out["mild_rot_excess_rad"] = max(out["mild_rot_excess_rad"], er)
    return out
