"""Inputs and recorded figures of the rig map-reconstruction tests (tests/test_map_rig_ref.py on the CPU,
tests/test_gpu_map_rig.py on the device): camera-major asl_obs blocks (n_cams, n_frames, max_tags) of the bench scene seen by
rigs with known mountings (rig_cases.exact_block with the true pose in every slot, as map_cases has it).  Every figure here
was measured on the CPU with the NumPy statement (tests/map_ref.py) -- never with the kernels; test_map_rig_ref.py
measures them again."""
import functools

import numpy as np

import localize_cases as LC
import map_cases as MC
import map_ref as MR
import rig_cases as RC
import smooth_rig_cases as SRC
from aprilslam_amd import _lib
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

TAG = LC.TAG_INNER
N_IDS = MC.N_IDS
PAIR = SRC.PAIR
HUBER = 1.0
NOISE = 0.3
ITERS = 60
COMPARE_ITERS = 3           # map_robust_cases' rule for a case whose trial count the rounding of its tail decides
MIN_MARGIN = 1e-6           # px: every corner of every trial of a compared case is at least this far from the threshold
SPLIT_ID = 10               # camera 0 keeps the ids below it, camera 1 the others
FRAME_CASE_SHAPE = (6, 12)  # frames x max_tags of the block the frame cases are cut from
# Its noise seed.  The LM stops at an accepted trial whose relative decrease is below 1e-12.  Where the statement's last
# accepted decrease is near 1e-14, the rounding of the cost sum decides whether that trial is accepted at all and with it
# the trial count (measured on the statement: with seed 5 the last decrease is 4e-15 to 5e-14, and 9 of 18 one-slot
# variants of the block change their trial count when the sums are reversed); a decrease near 1e-12 straddles the stop.
# The seed is the first from 5 on for which, plain and at HUBER, the last accepted decrease lies in [1e-13, 5e-13] and the
# one before it is >= 1e-11 (23: 2.1e-11, then 4.4e-13, 15 trials).
FRAME_CASE_SEED = 23
LONE_FRAME = 3              # by the same criterion among the six frames (9.9e-10, then 3.9e-13)


@functools.lru_cache(maxsize=None)
def scene():
    return TagMap.from_scene(LC.bench_scene())


def bench_poses(n=12, per_round=24):
    """world<-rig: the first n poses of the bench trajectory"""
    return [LC.world_from_camera(p, r) for p, r in LC.trajectory(per_round)[:n]]


def add_noise(obs, noise=NOISE, seed=5):
    """Gaussian corner noise drawn as map_robust_cases.noisy_block draws it: for the slots that hold a tag, in block order"""
    rng = np.random.default_rng(seed)
    out = obs.copy()
    held = out["id"] >= 0
    out["corners"][held] += rng.normal(0, noise, (int(held.sum()), 8)).astype(np.float32)
    return out


def keep(obs, mask):
    """obs with the slots outside mask emptied"""
    out = obs.copy()
    out["id"][~mask] = -1
    out["flags"][~mask] = 0
    return out


@functools.lru_cache(maxsize=None)
def pair_block(n_frames=12, max_tags=24, noise=0.0, seed=5):
    """the two-camera rig PAIR along the bench trajectory: 392 views of 240 (frame, tag) pairs at 12 x 24"""
    obs = RC.exact_block(scene(), PAIR, bench_poses(n_frames), TAG, max_tags, pnp_seed=None)
    return add_noise(obs, noise, seed) if noise else obs


def split(obs, split_id=SPLIT_ID):
    """camera 0 masked to the ids below split_id, camera 1 to the others: no tag is seen by both"""
    m = obs["id"] >= 0
    m[0] &= obs["id"][0] < split_id
    m[1] &= obs["id"][1] >= split_id
    return keep(obs, m)


def one_view_per_pair(obs):
    """every (frame, id) pair keeps its first view, in (camera, slot) order"""
    m = obs["id"] >= 0
    for f in range(obs.shape[1]):
        seen = set()
        for c in range(obs.shape[0]):
            for s in range(obs.shape[2]):
                if m[c, f, s]:
                    i = int(obs["id"][c, f, s])
                    m[c, f, s] = i not in seen
                    seen.add(i)
    return keep(obs, m)


def view_counts(obs):
    """(views, (frame, id) pairs) among the slots that hold a tag"""
    c, f, s = np.nonzero(obs["id"] >= 0)
    return len(c), len({(int(a), int(obs["id"][b, a, d])) for b, a, d in zip(c, f, s)})


MIXED = Rig([RigCamera(RC.K45, None, RC.mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(RC.K60, RC.DIST5, RC.mounting(5.0, (4.0, 0.5, 0.0)))])
MIXED_SIZES = [(LC.W, LC.H), (640, 480)]


@functools.lru_cache(maxsize=None)
def mixed_block(noise=0.0):
    """rig_cases' mixed_models rig (K45 + K60 / DIST5) on the same poses"""
    obs = RC.exact_block(scene(), MIXED, bench_poses(12), TAG, 24, sizes=MIXED_SIZES, pnp_seed=None)
    return add_noise(obs, noise) if noise else obs


def swap_slot(obs, c, f, s):
    """slot (c, f, s) carries slot s + 1's corners (a mis-decoded id), as map_robust_cases.swap"""
    out = obs.copy()
    assert obs["id"][c, f, s] >= 0 and obs["id"][c, f, s + 1] >= 0
    out["corners"][c, f, s] = obs["corners"][c, f, s + 1]
    return out


SWAPPED = (1, 6, 7)         # camera, frame, slot of the swapped-slot case


def truth_errors(out, poses, world_id=None):
    """largest tag translation error (scene units), tag rotation error (rad) and rig translation error of a statement or
    device output against the scene and the world<-rig poses, in the output's gauge"""
    tm = scene()
    w = int(out[0]["world_id"]) if world_id is None else world_id
    Gi = MR.inv(tm[w])
    et = er = ec = 0.0
    for i in np.flatnonzero(out[1]["valid"]):
        d = MR.inv(Gi @ tm[int(i)]) @ MR.rec4(out[1]["T"][i])
        et = max(et, float(np.linalg.norm(d[:3, 3])))
        er = max(er, float(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))))
    for f, T in enumerate(poses):
        if out[3]["status"][f] == 0:
            ec = max(ec, float(np.linalg.norm((Gi @ T)[:3, 3] - out[3]["T"][f][:3, 3])))
    return et, er, ec


def run(obs, rig, huber=0.0, max_iters=ITERS, reverse=False, trace=None, with_std=True, world_id=-1):
    return MR.map_rig_frames(obs, N_IDS, rig, TAG, world_id=world_id, huber_px=huber, max_iters=max_iters, trace=trace, reverse=reverse,
                         with_std=with_std)


def single(obs, c, rig=PAIR, world_id=-1, max_iters=ITERS):
    """the single-camera statement (map_ref.map_frames) on camera c's stream"""
    cam = rig.cameras[c]
    return MR.map_frames(obs[c], N_IDS, cam.K, cam.dist if len(cam.dist) else None, TAG, world_id=world_id, max_iters=max_iters)


# ---- the small and edge shapes of the device comparison
def empty(n_cams, n_frames, max_tags):
    e = np.zeros((n_cams, n_frames, max_tags), dtype=_lib.OBS_DTYPE)
    e["id"] = -1
    return e


def shape_block(n_cams, max_tags, n_frames=4):
    """(obs, rig): smooth_rig_cases.ring(n_cams) (one camera: the identity mounting) with max_tags slots a camera"""
    rig = Rig([RigCamera(RC.K45, None, np.eye(4))]) if n_cams == 1 else SRC.ring(n_cams)
    return add_noise(RC.exact_block(scene(), rig, bench_poses(n_frames), TAG, max_tags, pnp_seed=None)), rig


def behind_case():
    """(obs, rig): a pair whose first view the behind test drops while its second stays.  rig_cases' back-to-back rig, exact
    data: camera 0 looks along the rig's +z, camera 1 along -z, each sees its own two tags.  Frame 1's camera 0 gets a third
    slot, without a PnP pose (flags 1), that claims tag 2, which is in front of camera 1 and so behind camera 0: it costs
    4e12 under every candidate of the seeding, where it changes no choice (with the true pose in every slot the candidates
    are the same pose and the data are exact), the behind test drops it, and tag 2's pair in frame 1 is left with camera 1's
    view as its entry."""
    tm, rig, poses = RC.back_to_back()
    obs = RC.exact_block(tm, rig, poses, TAG, 4, pnp_seed=None)
    assert obs["id"][0, 1, 2] == -1 and 2 in obs["id"][1, 1]
    s = int(np.flatnonzero(obs["id"][1, 1] == 2)[0])
    obs[0, 1, 2] = obs[1, 1, s]
    obs["flags"][0, 1, 2] = 1
    return obs, rig


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (obs, rig)"""
    cases = {}
    two = pair_block(2, 24, NOISE)
    cases["2x2"] = (keep(two, np.isin(two["id"], sorted({int(i) for i in two["id"][0, 0] if i >= 0} & {int(i) for i in two["id"][0, 1] if i >= 0})[:2])), PAIR)
    for nc, mt in ((3, 5), (2, 8), (1, 17), (16, 16), (8, 32)):     # 15 / 16 / 17 global slots: a wavefront round of corners; 256
        cases["slots_%dx%d" % (nc, mt)] = shape_block(nc, mt, 3 if nc * mt == 256 else 4)
    big = pair_block(12, 24, NOISE)
    m = big["id"] >= 0
    for i, n in ((3, 16), (4, 17)):                                 # a tag's view list of 16 and of 17: map_tag_pass's round edge
        c, f, s = np.nonzero(big["id"] == i)
        order = np.lexsort((s, c, f))
        assert len(order) >= n
        for k in order[n:]:
            m[c[k], f[k], s[k]] = False
    cases["list_16_17"] = (keep(big, m), PAIR)
    six = pair_block(FRAME_CASE_SHAPE[0], FRAME_CASE_SHAPE[1], NOISE, FRAME_CASE_SEED)
    cases["disjoint"] = (split(six, 4), PAIR)
    only = six.copy()
    only[1] = empty(1, six.shape[1], six.shape[2])[0]
    cases["one_camera_sees"] = (only, PAIR)
    lone = six.copy()                                               # frame LONE_FRAME: one tag, seen by both cameras, and nothing else
    both = sorted({int(i) for i in six["id"][0, LONE_FRAME] if i >= 0} & {int(i) for i in six["id"][1, LONE_FRAME] if i >= 0})[0]
    keep2 = six["id"][:, LONE_FRAME] == both
    lone["id"][:, LONE_FRAME][~keep2], lone["flags"][:, LONE_FRAME][~keep2] = -1, 0
    cases["lone_pair_frame"] = (lone, PAIR)
    e = empty(2, 2, six.shape[2])
    cases["empty_first"] = (np.concatenate([e, six], axis=1), PAIR)
    cases["empty_middle"] = (np.concatenate([six[:, :3], e, six[:, 3:]], axis=1), PAIR)
    cases["empty_last"] = (np.concatenate([six, e], axis=1), PAIR)
    three = Rig(PAIR.cameras + [RigCamera(RC.K45, None, RC.mounting(20.0, (9.0, 0.0, 0.0)))])
    cases["blind_camera"] = (np.concatenate([six, empty(1, six.shape[1], six.shape[2])]), three)
    rep = six.copy()                                                # an id repeated inside camera 0's frame 1; both cameras hold it
    i0 = sorted({int(i) for i in six["id"][0, 1] if i >= 0} & {int(i) for i in six["id"][1, 1] if i >= 0})[0]
    s0 = int(np.flatnonzero(six["id"][0, 1] == i0)[0])
    assert six["id"][0, 1, s0 + 2] >= 0
    rep["id"][0, 1, s0 + 2] = i0                                    # a later slot of the camera claims the id too: it takes no part
    cases["repeated_id"] = (rep, PAIR)
    cases["behind"] = behind_case()
    return cases


def main_cases():
    """name -> (obs, rig): the split, overlap and mixed-model blocks with NOISE"""
    return {"split": (split(pair_block(12, 24, NOISE)), PAIR), "overlap": (pair_block(12, 24, NOISE), PAIR), "mixed_models": (mixed_block(NOISE), MIXED)}


def compared_cases():
    """(name, obs, rig, huber, max_iters) of every case the device is compared on"""
    out = []
    for n, (obs, rig) in main_cases().items():
        out += [(n, obs, rig, 0.0, ITERS), (n, obs, rig, HUBER, ITERS)]
    for n, (obs, rig) in edge_cases().items():
        for hub in (0.0, HUBER):
            out.append((n, obs, rig, hub, COMPARE_ITERS if (n, hub) in TAIL_CASES else ITERS))
    return out


def distance(a, b):
    """largest LC.rel_err between two outputs' valid tag poses and frame poses (map_robust_cases.distance)"""
    assert np.array_equal(a[1]["valid"], b[1]["valid"])
    return max([LC.rel_err(MR.rec4(x), MR.rec4(y)) for x, y, v in zip(a[1]["T"], b[1]["T"], a[1]["valid"]) if v] +
               [LC.rel_err(x, y) for x, y in zip(a[3]["T"], b[3]["T"])] + [0.0])


# ---- recorded figures (the statement's, measured on the CPU; test_map_rig_ref.py measures them again)
# Split case at NOISE: largest tag translation error of the rig solve and of the two single-camera solves (gauges 0 and 10).
SPLIT_ERRORS = {"rig": 0.8766, "camera0": 0.8307, "camera1": 0.5090}
# Overlap case at NOISE: mean tag std (all six components, mapped tags but the world tag) with every view in the solve and
# with one view per pair.
OVERLAP_STD = {"all_views": 0.3190, "one_per_pair": 0.3645}
# Swapped slot SWAPPED of camera 1 in the overlap block: largest tag translation error plain and at HUBER
SWAP_ERRORS = {"plain": 1.070e4, "robust": 0.9023}
# Clean slots the statement itself reports soft at HUBER beside the swapped one, as map_robust_cases.EXTRA_SOFT: the three
# (camera, frame, slot) that are soft in the overlap block without any swap too, each with one corner at 1.02 to 1.14 px
# (weights 0.87 to 0.98) under NOISE.
EXTRA_SOFT = [(0, 4, 2), (1, 0, 1), (1, 7, 1)]
# Bound of the device against the statement (map_robust_cases.DEVICE_TOL's rule): ten times the largest distance between
# the statement and the statement with its sums over the views reversed, over compared_cases(), floor 1e-9.
# Measured: 1.84e-13 at "behind" (exact data: 60 trials at the rounding floor of the cost); 1.12e-14 over the others.
DEVICE_TOL_MEASURED = 1.84e-13
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)
# (case, huber) whose trial count that reversal changes: compared at COMPARE_ITERS trials; their converged results moved by
# the distance beside them, and the converged device result must lie within ten times that of the converged statement.
TAIL_CASES = {("slots_2x8", 0.0): 1.70e-12, ("slots_2x8", HUBER): 1.70e-12, ("slots_8x32", HUBER): 3.15e-14,
              ("one_camera_sees", 0.0): 5.60e-9, ("one_camera_sees", HUBER): 5.60e-9}
