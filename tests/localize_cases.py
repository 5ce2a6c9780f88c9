"""Inputs of the localisation tests (tests/test_localize_ref.py on the CPU, tests/test_gpu_localize.py on the device):
asl_obs blocks built from exact projections of a known camera, and the ground-truth helpers."""
import numpy as np

import localize_ref as LR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import TagMap

W, H = 1280, 720
TAG_OUTER, TAG_INNER = 18.0, 10.0   # bench.py's scene: outer square rendered, inner square = the PnP size
SCENE_SEED = 20250620 + 1
MM_PER_UNIT = 55.6 / 10.0           # bench.py
FLIP4 = np.diag([1.0, -1.0, -1.0, 1.0])


def bench_scene(width=W, height=H, ntags=20):
    return synth.random_scene(width, height, ntags, np.random.default_rng(SCENE_SEED), tag_size_outer=TAG_OUTER)


def world_from_camera(pos, rot):
    """ground truth world<-camera (OpenCV camera) of synth's camera at (pos, rot) in the scene's world frame"""
    return np.linalg.inv(FLIP4 @ synth.view_matrix(pos, rot))


def trajectory(n):
    """bench.camera_trajectory"""
    out = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1)
        out.append(((1.5 * np.cos(a), 1.0 * np.sin(a), 2.0 * np.sin(2 * a)), (0.6 * np.sin(a), 0.8 * np.cos(a), 0.5 * np.sin(3 * a))))
    return out


def exact_frame(tags, pos, rot, K, dist=None, tag_size=TAG_INNER, max_tags=None, width=W, height=H):
    """one frame's asl_obs row: every tag in front of the camera whose corners project inside the image, corners
    projected exactly (then rounded to float32 as the records hold them), T = the true camera<-tag"""
    cam = LR.camera(K, dist)
    obj = np.c_[LR.object_corners(tag_size), np.zeros(4)]
    rows = []
    for tag in sorted(tags, key=lambda t: t["id"]):
        T = synth.camera_from_tag(tag["position"], tag["rotation"], pos, rot)
        P = obj @ T[:3, :3].T + T[:3, 3]
        if np.any(P[:, 2] <= 1e-3):
            continue
        uv = LR.project(cam, P)
        if np.any(uv < 0) or np.any(uv[:, 0] >= width) or np.any(uv[:, 1] >= height):
            continue
        rows.append((int(tag["id"]), uv, T))
    n = max_tags or max(1, len(rows))
    obs = np.zeros(n, dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    for k, (i, uv, T) in enumerate(rows[:n]):
        obs["id"][k] = i
        obs["flags"][k] = 3
        obs["corners"][k] = uv.ravel()
        obs["T"][k] = T.ravel()[:12]
    return obs


def mirror_all(obs):
    """every seeding slot's PnP pose replaced by its mirrored planar minimum"""
    out = obs.copy()
    for idx in zip(*np.nonzero(out["flags"] & 2)):
        T = np.eye(4)
        T[:3] = out["T"][idx].reshape(3, 4)
        R, t = LR.mirrored(T[:3, :3], T[:3, 3])
        out["T"][idx] = np.c_[R, t].ravel()
    return out


def rot_err(Ta, Tb):
    R = Ta[:3, :3] @ Tb[:3, :3].T
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def rel_err(Ta, Tb):
    return float(np.abs(np.asarray(Ta) - np.asarray(Tb)).max() / max(1.0, np.abs(Tb).max()))


def cpu_cases(K):
    """(name, obs (n_frames, max_tags), TagMap records, dist, gate) of the CPU statement tests, for the kernel comparison"""
    tags = bench_scene()
    tm = TagMap.from_scene(tags)
    rec = tm.as_records()
    cams = trajectory(16)[:8]
    plain = np.stack([exact_frame(tags, p, r, K, max_tags=24) for p, r in cams])
    cases = [("exact", plain, rec, None, 0.0), ("mirrored", mirror_all(plain), rec, None, 0.0)]
    moved = tm.as_records()
    moved["T"][7][3] += 5.0                    # tag 7 moved 5 units along world x
    cases.append(("gate", plain, moved, None, 2.0))
    cases.append(("gate_off", plain, moved, None, 0.0))
    odd = plain.copy()
    odd["flags"][0] = 0                        # frame 0: no slot taking part -> status 1
    odd["flags"][1] = np.where(odd["id"][1] >= 0, 1, 0)     # frame 1: nothing with a PnP -> status 2
    odd["id"][2, ::3] = -1                     # frame 2: empty slots in between
    odd["flags"][2, ::3] = 0
    odd["flags"][3, 1::2] &= 1                 # frame 3: PnP-failed slots (residuals, no seeds)
    odd["id"][4, :5] = 999                     # frame 4: ids outside the map
    cases.append(("slots", odd, rec, None, 0.0))
    for nd, dist in ((4, np.array([-0.08, 0.03, 0.0008, -0.0006])), (5, np.array([-0.12, 0.05, 0.001, -0.0015, 0.01]))):
        obs = np.stack([exact_frame(tags, p, r, K, dist=dist, max_tags=24) for p, r in cams[:4]])
        cases.append(("dist%d" % nd, obs, rec, dist, 0.0))
    return cases
