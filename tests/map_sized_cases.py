"""Inputs and recorded figures of the sized tag-map reconstruction tests (tests/test_map_sized_ref.py on the CPU,
tests/test_gpu_map_sized.py on the device): asl_obs blocks of scenes whose tags have different known sizes, built with
sized_cases.block (exact projections at the true sizes, records as a PnP at the call's tag_size gives them), at most
12 frames x 24 slots.  Every figure here was measured on the CPU with the NumPy statement (tests/map_ref.py) -- never
with the kernels; test_map_sized_ref.py measures them again."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import map_ref as MR
import map_rig_cases as GC
import rig_cases as RC
import sized_cases as SC
import smooth_rig_cases as SRC
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

TAG = SC.TAG
N_IDS = GC.N_IDS
RATIOS = SC.RATIOS
HUBER = GC.HUBER
NOISE = GC.NOISE
ITERS = GC.ITERS
COMPARE_ITERS = GC.COMPARE_ITERS
MIN_MARGIN = GC.MIN_MARGIN
PAIR = GC.PAIR
SOLO = Rig([RigCamera(RC.K45, None, np.eye(4))])
FLIP_TAG = 15
# Noise seeds, by map_rig_cases' criterion (FRAME_CASE_SEED) on every case with noise: the first from 5 on for which, plain and
# at HUBER, the statement's last accepted relative decrease lies in [1e-13, 5e-13] and the one before it is >= 1e-11, so that
# the rounding of the cost sums does not decide the trial count.
SEEDS = {"single_mixed": 5, "pair_mixed": 15, "all_sized": 5, "slots_3x5": 5, "slots_2x8": 8, "slots_1x17": 19, "list_16_17": 16, "mirrored_sweep": 16}


def table(sizes):
    """(N_IDS,) float32 from {id: size}"""
    t = np.zeros(N_IDS, dtype=np.float32)
    for i, s in sizes.items():
        t[i] = s
    return t


def sized_scene(sizes):
    """the bench scene (map_rig_cases.scene) with the sizes {id: side} on its tags; ids outside it are left out"""
    tm = GC.scene()
    return TagMap(tm.poses, {i: s for i, s in sizes.items() if i in tm.poses})


def mixed_sizes():
    """every third id of the bench scene from the world tag 0 on, across RATIOS (0: 0.25 TAG, 3: 0.5, 6: 1.5, 9: 2, 12: 3,
    15: 4, 18: 0.25), and entries for ids the scene does not have (40..63: 2 TAG)"""
    s = {i: TAG * RATIOS[k % len(RATIOS)] for k, i in enumerate(range(0, 20, 3))}
    s.update({i: 2 * TAG for i in range(40, N_IDS)})
    return s


def all_sizes():
    return {i: TAG * RATIOS[i % len(RATIOS)] for i in GC.scene().ids()}


def build(sizes, rig, n_frames, max_tags, noise=NOISE, seed=5, poses=None):
    """(obs, rig, table): the sized bench scene seen by rig along the bench trajectory, true pose in every record (its
    translation over k for a sized tag), corner noise as map_rig_cases.add_noise draws it"""
    obs = SC.block(sized_scene(sizes), rig, poses or GC.bench_poses(n_frames), TAG, max_tags, pnp_seed=None)
    return (GC.add_noise(obs, noise, seed) if noise else obs), rig, table(sizes)


def mirrored_sweep_case(seed):
    """(obs, rig, table): the pair's mixed block, 6 x 12; in frame 2 only the sized views may seed and their records hold the
    mirrored planar minimum: the chain places the frame from one of them and the frame sweep's winner is the mirrored
    candidate of a sized view (the true pose)"""
    obs, rig, t = build(mixed_sizes(), PAIR, 6, 12, seed=seed)
    obs = obs.copy()
    f = 2
    for c in range(obs.shape[0]):
        for s in range(obs.shape[2]):
            i = int(obs["id"][c, f, s])
            if i < 0:
                continue
            if t[i] > 0:
                T = obs["T"][c, f, s].reshape(3, 4)
                R, tt = LR.mirrored(T[:, :3], T[:, 3])
                obs["T"][c, f, s] = np.c_[R, tt].ravel()
            else:
                obs["flags"][c, f, s] &= 1
    return obs, rig, t


def flip_case():
    """(obs, rig, table): map_cases.flip_case's recipe with tag FLIP_TAG of side 2 TAG, one camera: 6 frames of a short
    baseline; the tag's records all hold the multi-view second minimum of its pose (at its own half, the translation over
    k as a PnP at TAG gives it) and only its smallest view may seed"""
    sizes = {FLIP_TAG: 2 * TAG, 3: 0.5 * TAG}
    poses = [LC.world_from_camera(p, r) for p, r in LC.trajectory(256)[:6]]
    obs, rig, t = build(sizes, SOLO, 6, 24, noise=0.0, poses=poses)
    obs = obs.copy()
    tm = sized_scene(sizes)
    h, half = LR.size_half(t[FLIP_TAG], TAG)[0], LR.half_size(TAG)
    W = [MR.inv(T) for T in poses]
    views = [(LR.corner_area(obs["corners"][0, f, s]), f, s) for f, s in zip(*np.nonzero(obs["id"][0] == FLIP_TAG))]
    _, b, _ = max(views, key=lambda v: (v[0], -v[1]))
    tab = MR.rig_ref.rig_table(rig)
    G2, _ = MR.tag_lm(tab, [0] * len(views), MR.inv(W[b]) @ MR.mirror4(W[b] @ tm[FLIP_TAG]), [W[f] for _, f, _ in views],
                      [obs["corners"][0, f, s].astype(np.float64).reshape(4, 2) for _, f, s in views], h)
    for _, f, s in views:
        T = (W[f] @ G2)[:3].copy()
        T[:, 3] = T[:, 3] / (h / half)
        obs["T"][0, f, s] = T.ravel()
        obs["flags"][0, f, s] = 1
    _, f1, s1 = min(views, key=lambda v: (v[0], v[1]))
    obs["flags"][0, f1, s1] = 3
    return obs, rig, t


def behind_case():
    """(obs, rig, table): map_rig_cases.behind_case with the claimed tag 2 of side 2 TAG"""
    tm, rig, poses = RC.back_to_back()
    sizes = {2: 2 * TAG, 0: 0.5 * TAG}
    obs = SC.block(TagMap(tm.poses, sizes), rig, poses, TAG, 4, pnp_seed=None)
    assert obs["id"][0, 1, 2] == -1 and 2 in obs["id"][1, 1]
    s = int(np.flatnonzero(obs["id"][1, 1] == 2)[0])
    obs[0, 1, 2] = obs[1, 1, s]
    obs["flags"][0, 1, 2] = 1
    return obs, rig, table(sizes)


def shape_case(n_cams, max_tags, seed):
    """(obs, rig, table): map_rig_cases.shape_block's rig and poses; every id % 4 == 1 is sized, and so is the id in frame 0's
    last global slot (at 1 x 17 that is global slot 16), of side 2 TAG.  A sized tag may enter or leave a camera's view, so
    the id is read from the block built with it"""
    rig = SOLO if n_cams == 1 else SRC.ring(n_cams)
    sizes = {i: TAG * RATIOS[i % len(RATIOS)] for i in GC.scene().ids() if i % 4 == 1}
    for _ in range(4):
        obs, rig, t = build(sizes, rig, 4, max_tags, seed=seed)
        last = int(obs["id"][n_cams - 1, 0, max_tags - 1])
        if t[last] == 2 * TAG:
            return obs, rig, t
        sizes[last] = 2 * TAG
    raise AssertionError("no sized tag settles in the last slot")


def list_case(seed):
    """(obs, rig, table): map_rig_cases' list_16_17 with the tags of 16 and of 17 views sized (ids 3 and 4)"""
    sizes = {3: 2 * TAG, 4: 0.5 * TAG, 0: 1.5 * TAG}
    big, rig, t = build(sizes, PAIR, 12, 24, seed=seed)
    m = big["id"] >= 0
    for i, n in ((3, 16), (4, 17)):
        c, f, s = np.nonzero(big["id"] == i)
        order = np.lexsort((s, c, f))
        assert len(order) >= n, (i, len(order))
        for k in order[n:]:
            m[c[k], f[k], s[k]] = False
    return GC.keep(big, m), rig, t


def noisy_case(name, seed):
    """(obs, rig, table) of the case with corner noise `name`, drawn with `seed`"""
    if name in ("single_mixed", "pair_mixed"):
        return build(mixed_sizes(), SOLO if name == "single_mixed" else PAIR, 12, 24, seed=seed)
    if name == "all_sized":
        return build(all_sizes(), PAIR, 6, 12, seed=seed)
    if name.startswith("slots_"):
        nc, mt = name[6:].split("x")
        return shape_case(int(nc), int(mt), seed)
    return {"list_16_17": list_case, "mirrored_sweep": mirrored_sweep_case}[name](seed)


@functools.lru_cache(maxsize=None)
def main_cases():
    """name -> (obs, rig, table): one camera and the pair on the mixed scene, 12 x 24"""
    return {n: noisy_case(n, SEEDS[n]) for n in ("single_mixed", "pair_mixed")}


@functools.lru_cache(maxsize=None)
def edge_cases():
    cases = {n: noisy_case(n, SEEDS[n]) for n in ("all_sized", "slots_3x5", "slots_2x8", "slots_1x17", "list_16_17", "mirrored_sweep")}
    cases["flip"] = flip_case()
    cases["behind"] = behind_case()
    return cases


def compared_cases():
    """(name, obs, rig, table, huber, max_iters) of every case the device is compared on"""
    out = []
    for n, (obs, rig, t) in main_cases().items():
        out += [(n, obs, rig, t, 0.0, ITERS), (n, obs, rig, t, HUBER, ITERS)]
    for n, (obs, rig, t) in edge_cases().items():
        for hub in (0.0, HUBER):
            out.append((n, obs, rig, t, hub, COMPARE_ITERS if (n, hub) in TAIL_CASES else ITERS))
    return out


def run(obs, rig, t, huber=0.0, max_iters=ITERS, reverse=False, trace=None, world_id=-1):
    return MR.map_rig_frames(obs, N_IDS, rig, TAG, t, world_id=world_id, huber_px=huber, max_iters=max_iters, trace=trace, reverse=reverse)


distance = GC.distance


# ---- the truth (sized_cases.truth_case: 6 tags, id 5 of side 2 TAG, 6 frames x 4 slots, exact corners and records)
def truth_case(sized=True):
    """(obs (1, 6, 4), table (6,), {id: world<-tag}, [world<-camera]) in the gauge of tag 0"""
    obs, rec, poses = SC.truth_case(sized)
    tm = SC.small_map(sized)
    Gi = MR.inv(tm[0])
    return obs[None], rec["size"].astype(np.float32), {i: Gi @ tm[i] for i in tm.ids()}, [Gi @ T for T in poses]


def truth_err(out, gt_tags, gt_poses):
    """largest LC.rel_err of the mapped tags and the frame poses against the truth"""
    return max([LC.rel_err(MR.rec4(out[1]["T"][i]), gt_tags[i]) for i in np.flatnonzero(out[1]["valid"])] +
               [LC.rel_err(p["T"], T) for p, T in zip(out[3], gt_poses)])


@functools.lru_cache(maxsize=None)
def truth_bar():
    """(the statement's error on the equal-size scene of truth_case's geometry, the bar: ten times it): sized_cases.truth_bar's
    rule"""
    obs, t, gt, gp = truth_case(sized=False)
    base = truth_err(MR.map_rig_frames(obs, 6, SC.one_camera(), TAG, t, max_iters=ITERS), gt, gp)
    return base, 10 * base


# ---- recorded figures (the statement's, measured on the CPU; test_map_sized_ref.py measures them again)
# truth_case through the statement: its error with the table, on the equal-size scene (truth_bar's base), and without the
# table on the sized block: the plain call's map has tag 5 at about half its distance
# (0.566: the largest relative pose error, tag 5 at 85.3 units from the world tag where it is 95.5 away)
TRUTH_ERRORS = {"sized": 4.94e-7, "equal": 3.47e-7, "plain": 0.566}
# Bound of the device against the statement (map_rig_cases.DEVICE_TOL's rule): ten times the largest distance between the
# statement and the statement with its view sums reversed, over compared_cases(), floor 1e-9.
# Measured: 8.55e-14 at the mirrored-sweep case with HUBER.
DEVICE_TOL_MEASURED = 8.55e-14
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)
# (case, huber) whose trial count that reversal changes: compared at COMPARE_ITERS trials; beside each the distance of the
# converged results, and the converged device result must lie within ten times that of the converged statement.
# With the seeds above there is none (at seed 5 slots_2x8 and slots_1x17 were, 1.3e-10 and 1.7e-9).
TAIL_CASES = {}
