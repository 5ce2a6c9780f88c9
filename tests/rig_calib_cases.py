"""Inputs of the rig mounting calibration tests (tests/test_rig_calib_ref.py on the CPU, tests/test_gpu_rig_calib.py on the
device), built from rig_cases: the blocks of known rigs, with the mountings of cameras 1 and up moved off the truth by a
seeded perturbation, or averaged from single-camera localisations (one_tag)."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import rig_cases as RC
from aprilslam_amd.rig import Rig, RigCamera

ROT_OFF_DEG, TRANS_OFF = 2.0, 0.5
ONE_TAG_NOISE_PX = 0.3
# the truth bound of one_tag: twice the statement's own worst error over seeds 0..4 (0.4200 degrees at seed 3, 0.4999 units at
# seed 4; tests/test_rig_calib_ref.py measures them and records every seed's figures)
ONE_TAG_ROT_DEG, ONE_TAG_TRANS = 2 * 0.4200, 2 * 0.4999
EXACT = ["pair", "mixed", "ring8", "dropout"]
NAMES = EXACT + ["one_tag", "island", "nothing"]


def perturbed(rig, seed):
    """the rig with the mounting of every camera but the first turned by ROT_OFF_DEG about a seeded axis and moved by
    TRANS_OFF along another"""
    rng = np.random.default_rng(seed)
    cams = [rig.cameras[0]]
    for c in rig.cameras[1:]:
        ax, dr = rng.normal(size=3), rng.normal(size=3)
        off = RC.transform(ax / np.linalg.norm(ax) * np.radians(ROT_OFF_DEG), dr / np.linalg.norm(dr) * TRANS_OFF)
        cams.append(RigCamera(c.K, c.dist, off @ c.T_cam_rig))
    return Rig(cams)


def cleared(obs, cams):
    """the block with every slot of the given cameras empty"""
    out = obs.copy()
    for c in cams:
        out["id"][c] = -1
        out["flags"][c] = 0
    return out


def noisy(obs, sigma, seed):
    out = obs.copy()
    rng = np.random.default_rng(seed)
    noise = rng.normal(size=out["corners"].shape) * sigma * (out["flags"] & 1)[..., None]
    out["corners"] = (out["corners"].astype(np.float64) + noise).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def _rig_cases():
    return {c["name"]: c for c in RC.cases()}


@functools.lru_cache(maxsize=None)
def one_tag(seed=0):
    """back_to_back(1, 120.0, 24): each camera sees one small tag of its own, corners noisy by ONE_TAG_NOISE_PX; the
    initial rig is Rig.from_camera_poses over the statement's single-camera localisations"""
    tm, rig, poses = RC.back_to_back(1, 120.0, 24)
    rec = tm.as_records()
    obs = noisy(RC.exact_block(tm, rig, poses, LC.TAG_INNER, 4), ONE_TAG_NOISE_PX, seed)
    single = [LR.localize(obs[c], rec, rc.K, rc.dist, LC.TAG_INNER) for c, rc in enumerate(rig.cameras)]
    rig0 = Rig.from_camera_poses([(rc.K, rc.dist) for rc in rig.cameras], single)
    return dict(name="one_tag", obs=obs, rec=rec, rig0=rig0, truth=rig, tag_size=LC.TAG_INNER, exact=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, obs, rec, rig0 (the initial rig), truth (the rig the block was made with), tag_size, exact)"""
    if name == "one_tag":
        return one_tag(0)
    src = {"pair": "side_by_side", "mixed": "mixed_models", "ring8": "slots_256", "dropout": "dropout", "island": "side_by_side",
           "nothing": "side_by_side"}[name]
    c = _rig_cases()[src]
    obs, truth = c["obs"], c["rig"]
    if name == "island":
        third = RigCamera(RC.K45, None, RC.mounting(20.0, (9.0, 0.0, 0.0)))
        truth = Rig(truth.cameras + [third])
        obs = np.concatenate([obs, cleared(obs[:1], [0])])
    if name == "nothing":
        obs = cleared(obs, range(1, obs.shape[0]))
    return dict(name=name, obs=np.ascontiguousarray(obs), rec=c["rec"], rig0=perturbed(truth, 11 + NAMES.index(name)), truth=truth,
                tag_size=c["tag_size"], exact=name in EXACT)
