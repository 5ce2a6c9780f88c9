"""Inputs of the rig localisation tests (tests/test_rig_ref.py on the CPU, tests/test_gpu_rig.py on the device): asl_obs
blocks (n_cams, n_frames, max_tags), camera-major, from exact projections of rigs with known mountings moved along known
poses, all built from 4x4 matrices with localize_ref.project."""
import numpy as np

import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

K45 = synth.camera_matrix(LC.W, LC.H, 45.0)
K60 = synth.camera_matrix(640, 480, 60.0)
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
FRONTAL = np.diag([1.0, -1.0, -1.0])      # camera<-tag rotation of a tag seen head-on


def transform(rvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    """4x4 [Rod(rvec) | t]"""
    T = np.eye(4)
    T[:3, :3] = LR.rodrigues(np.asarray(rvec, dtype=np.float64))
    T[:3, 3] = t
    return T


def mounting(yaw_deg=0.0, offset=(0.0, 0.0, 0.0), pitch_deg=0.0):
    """camera<-rig of a camera that sits at `offset` in the rig frame, turned by yaw about the rig's y and pitch about x"""
    rig_from_cam = transform((0.0, np.radians(yaw_deg), 0.0), offset) @ transform((np.radians(pitch_deg), 0.0, 0.0))
    return np.linalg.inv(rig_from_cam)


PNP_ROT_SIGMA, PNP_TRANS_REL_SIGMA = 0.02, 0.005   # the records' PnP poses are off the truth about as a single view is


def exact_block(tm, rig, poses, tag_size, max_tags, sizes=None, pnp_seed=1):
    """(n_cams, n_frames, max_tags) asl_obs: for camera c and frame f every map tag in front of the camera whose corners
    project inside its image (sizes[c] = (width, height), default LC.W x LC.H), in id order: corners projected exactly
    (rounded to float32 as the records hold them).  poses: world<-rig 4x4 per frame.  The record's T is the true
    camera<-tag moved by a small seeded error of its own (PNP_ROT_SIGMA rad, PNP_TRANS_REL_SIGMA of the distance), as every
    slot's single-view PnP has: with the true pose in every slot all candidates would be the same pose and their order a
    matter of rounding.  pnp_seed None: the true pose."""
    obj = np.c_[LR.object_corners(tag_size), np.zeros(4)]
    rng = np.random.default_rng(pnp_seed)
    obs = np.zeros((len(rig), len(poses), max_tags), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    for c, rc in enumerate(rig.cameras):
        cam = LR.camera(rc.K, rc.dist)
        w, h = sizes[c] if sizes else (LC.W, LC.H)
        for f, Twr in enumerate(poses):
            Tcw = rc.T_cam_rig @ np.linalg.inv(Twr)
            k = 0
            for i in tm.ids():
                T = Tcw @ tm[i]
                P = obj @ T[:3, :3].T + T[:3, 3]
                if np.any(P[:, 2] <= 1e-3):
                    continue
                uv = LR.project(cam, P)
                if np.any(uv < 0) or np.any(uv[:, 0] >= w) or np.any(uv[:, 1] >= h) or k >= max_tags:
                    continue
                if pnp_seed is not None:
                    T = transform(rng.normal(size=3) * PNP_ROT_SIGMA, rng.normal(size=3) * PNP_TRANS_REL_SIGMA * np.linalg.norm(T[:3, 3])) @ T
                obs[c, f, k] = (i, 3, uv.ravel(), T.ravel()[:12])
                k += 1
    return obs


def synth_camera(T_wc):
    """(position, rotation in degrees) of synth's camera whose world<-camera (OpenCV camera, LC.world_from_camera) is T_wc:
    view_matrix's rotation Rz(-roll) Rx(-pitch) Ry(-yaw) taken apart, so that a camera mounted on a rig can be rendered"""
    V = LC.FLIP4 @ np.linalg.inv(T_wc)
    M = V[:3, :3]
    b = np.arcsin(np.clip(M[2, 1], -1.0, 1.0))
    c = np.arctan2(-M[2, 0], M[2, 2])
    a = np.arctan2(-M[0, 1], M[1, 1])
    pos = -(M.T @ V[:3, 3])
    return tuple(pos), tuple(np.degrees([-b, -c, -a]))


def bench_poses(n=6):
    """world<-rig along the bench trajectory"""
    return [LC.world_from_camera(p, r) for p, r in LC.trajectory(16)[:n]]


def back_to_back(tags_per_side=2, distance=120.0, n_frames=6, seed=3):
    """(TagMap, Rig, poses): camera 0 looks along the rig's +z, camera 1 along -z; tags_per_side tags of side LC.TAG_INNER
    in front of each at `distance` (about 72 px across at 120), tilted 20..40 degrees; the rig moves a little about the
    world origin"""
    rng = np.random.default_rng(seed)
    rig = Rig([RigCamera(K45, None, np.eye(4)), RigCamera(K45, None, mounting(180.0))])
    tm = TagMap()
    for c in range(2):
        for k in range(tags_per_side):
            ax = rng.normal(size=3)
            Tct = np.eye(4)
            Tct[:3, :3] = LR.rodrigues(ax / np.linalg.norm(ax) * np.radians(rng.uniform(20, 40))) @ FRONTAL
            x = (k - (tags_per_side - 1) / 2) * 0.5 * distance
            Tct[:3, 3] = [x, rng.uniform(-0.1, 0.1) * distance, distance * rng.uniform(0.9, 1.1)]
            tm[c * tags_per_side + k] = np.linalg.inv(rig.cameras[c].T_cam_rig) @ Tct      # world = the rig at rest
    poses = [transform(rng.normal(size=3) * 0.03, rng.normal(size=3) * 2.0) for _ in range(n_frames)]
    return tm, rig, poses


def cases():
    """[dict(name, obs (n_cams, n_frames, max_tags), rec (map records), rig, tag_size, gate, truth (n_frames world<-rig))]"""
    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    rec = tm.as_records()
    poses = bench_poses()
    ts = LC.TAG_INNER
    out = []

    def add(name, obs, rig, truth, rec_=rec, gate=0.0):
        out.append(dict(name=name, obs=obs, rec=rec_, rig=rig, tag_size=ts, gate=gate, truth=truth))

    pair = Rig([RigCamera(K45, None, mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(K45, None, mounting(7.0, (4.0, 0.5, 0.0), 2.0))])
    side = exact_block(tm, pair, poses, ts, 24)
    add("side_by_side", side, pair, poses)

    tm_bb, rig_bb, poses_bb = back_to_back()
    add("back_to_back", exact_block(tm_bb, rig_bb, poses_bb, ts, 4), rig_bb, poses_bb, rec_=tm_bb.as_records())

    drop = side.copy()
    drop["id"][1, 2:4] = -1                    # camera 1: nothing in view in frames 2 and 3
    drop["flags"][1, 2:4] = 0
    add("dropout", drop, pair, poses)

    add("mirror_all", LC.mirror_all(side), pair, poses)

    one = side.copy()
    one["flags"][0] &= 1                       # camera 0: corners only; camera 1: one slot with a pose
    one["flags"][1, :, 1:] &= 1
    add("one_seeder", one, pair, poses)

    mixed = Rig([RigCamera(K45, None, mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(K60, DIST5, mounting(5.0, (4.0, 0.5, 0.0)))])
    add("mixed_models", exact_block(tm, mixed, poses, ts, 24, sizes=[(LC.W, LC.H), (640, 480)]), mixed, poses)

    moved = tm.as_records()
    moved["T"][7][3] += 5.0                    # tag 7 moved 5 units along world x
    add("gate", side, pair, poses, rec_=moved, gate=2.0)

    ring = Rig([RigCamera(K45, None, mounting(-14.0 + 4.0 * c, (-7.0 + 2.0 * c, 0.3 * (c % 3), 0.0), 1.0 * (c % 2))) for c in range(8)])
    add("slots_256", exact_block(tm, ring, poses[:4], ts, 32), ring, poses[:4])

    solo = Rig([RigCamera(K45, None, np.eye(4))])
    add("single", exact_block(tm, solo, poses, ts, 24), solo, poses)
    return out


def case(name):
    return [c for c in cases() if c["name"] == name][0]


NAMES = ["side_by_side", "back_to_back", "dropout", "mirror_all", "one_seeder", "mixed_models", "gate", "slots_256", "single"]
