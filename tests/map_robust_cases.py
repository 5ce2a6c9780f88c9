"""Inputs of the robust map-reconstruction tests (tests/test_map_robust_ref.py on the CPU, tests/test_gpu_map_robust.py on
the device): map_cases' exact blocks with 0.3 px of corner noise and a few corrupted slots, the small and edge shapes, and the
statement's recorded errors."""
import functools

import numpy as np

import localize_cases as LC
import map_cases as MC
import map_ref as MR

K = MC.K_bench()
HUBER = 1.0
NOISE = 0.3
ITERS = 60
COMPARE_ITERS = 3           # for a case whose trial count the rounding of its tail decides (smooth_cases.COMPARE_ITERS' rule)
MIN_MARGIN = 1e-6           # px: every corner of every trial of a compared case is at least this far from the threshold


def noisy_block(n_frames=12, max_tags=24, dist=None, noise=NOISE, seed=5):
    """(obs, tags, cams): map_cases.exact_block with Gaussian corner noise, drawn for the slots that hold a tag, in
    (frame, slot) order (the empty slots take no draws)"""
    obs, tags, cams = MC.exact_block(n_frames, dist=dist, max_tags=max_tags, K=K)
    rng = np.random.default_rng(seed)
    obs = obs.copy()
    held = obs["id"] >= 0
    obs["corners"][held] += rng.normal(0, noise, (int(held.sum()), 8)).astype(np.float32)
    return obs, tags, cams


def slip(obs, f, s, d=(12.0, 12.0)):
    """corner 0 of slot (f, s) moved by d pixels"""
    out = obs.copy()
    out["corners"][f, s, 0] += np.float32(d[0])
    out["corners"][f, s, 1] += np.float32(d[1])
    return out


def swap(obs, slots, with_pose=False):
    """every slot (f, s) of slots carries slot s + 1's corners (a mis-decoded id); with_pose: and its PnP pose"""
    out = obs.copy()
    for f, s in slots:
        assert obs["id"][f, s] >= 0 and obs["id"][f, s + 1] >= 0
        out["corners"][f, s] = obs["corners"][f, s + 1]
        if with_pose:
            out["T"][f, s] = obs["T"][f, s + 1]
    return out


def seed_slot_of(obs, f):
    return int(MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, max_iters=1, with_std=False)[3]["seed_slot"][f])


# ---- the repair cases: name -> (obs, tags, cams, dist, corrupted slots)
@functools.lru_cache(maxsize=None)
def repair_cases():
    big, tags, cams = noisy_block(12, 24)
    small, stags, scams = noisy_block(6, 8)
    d5, dtags, dcams = noisy_block(12, 24, dist=MC.DIST5)
    s3 = seed_slot_of(big, 3)
    return {
        "noise": (big, tags, cams, None, []),
        "slip": (slip(big, 6, 0), tags, cams, None, [(6, 0)]),
        "swap": (swap(big, [(6, 10)]), tags, cams, None, [(6, 10)]),
        "swap3": (swap(big, [(2, 3), (6, 10), (9, 17)]), tags, cams, None, [(2, 3), (6, 10), (9, 17)]),
        "seed_slip": (slip(big, 3, s3), tags, cams, None, [(3, s3)]),
        "small_noise": (small, stags, scams, None, []),
        "small_slip": (slip(small, 3, 0), stags, scams, None, [(3, 0)]),
        "small_swap": (swap(small, [(3, 2)]), stags, scams, None, [(3, 2)]),
        "dist5_swap": (swap(d5, [(6, 10)]), dtags, dcams, MC.DIST5, [(6, 10)]),
    }


def seed_swap_case():
    """frame 3's seed slot carries the next tag's corners and PnP pose: the seeding's limit, recorded and not barred"""
    big, tags, cams = noisy_block(12, 24)
    s3 = seed_slot_of(big, 3)
    return swap(big, [(3, s3)], with_pose=True), tags, cams, None, [(3, s3)]


# The statement's errors against the truth (map_cases.map_errors: largest tag translation, tag rotation, camera
# translation) at HUBER and ITERS, measured; every bar is twice the measured value (test_rectify_ref.py's rule).
#                 tag translation, tag rotation (rad), camera translation
ROBUST_MEASURED = {
    "noise": (1.355, 0.03353, 2.112),
    "slip": (1.357, 0.03229, 2.325),
    "swap": (1.353, 0.03352, 2.135),
    "swap3": (1.360, 0.03296, 2.133),
    "seed_slip": (1.336, 0.03216, 2.264),
    "small_noise": (0.8877, 0.05492, 0.9131),
    "small_slip": (1.833, 0.0607, 1.154),
    "small_swap": (0.8724, 0.05719, 0.9072),
    "dist5_swap": (1.434, 0.03726, 2.28),
}
# the plain statement on the same inputs, for the repair conditions (plain >= 3 x noise-only, robust <= 1.5 x noise-only)
PLAIN_MEASURED = {
    "noise": (1.355, 0.03353, 2.112),
    "slip": (8.647, 0.06269, 5.37),
    "swap": (127.7, 0.7923, 90.92),
    "swap3": (1.561e4, 1.188, 184.1),
    "seed_slip": (8.607, 0.06298, 5.478),
    "small_noise": (0.8877, 0.05492, 0.9131),
    "small_slip": (18.16, 0.115, 10.4),
    "small_swap": (3031.0, 0.6371, 100.6),
    "dist5_swap": (125.4, 0.7721, 88.16),
}
# the seed-slot swap, robust (44 soft slots, 17 trials) and plain (60 trials): the baseline for later work on the
# seeding; not a bar
SEED_SWAP_MEASURED = {"robust": (1.322, 1.821, 2.08), "plain": (537.3, 1.91, 462.1)}
# The soft slots of a case at HUBER are its corrupted slots, but for the slip in frame 3's seed slot: there the slipped
# corner bends frame 3's pose enough to put one corner of the frame's slot 10 at 1.0097 px (weight 0.99) as well.
EXTRA_SOFT = {"seed_slip": [(3, 10)]}
REPAIR_ROWS = ("slip", "swap", "swap3")


@functools.lru_cache(maxsize=None)
def statement(name, huber=HUBER, reverse=False, max_iters=ITERS):
    """(outputs of map_ref.map_frames, trace) of a repair case"""
    obs, _, _, dist, _ = repair_cases()[name]
    trace = {}
    out = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, huber_px=huber, max_iters=max_iters, trace=trace, reverse=reverse)
    return out, trace


def errors(name, out):
    _, tags, cams, _, _ = repair_cases()[name]
    return MC.map_errors(out[1], out[3], tags, cams, int(out[0]["world_id"]))


def soft_slots(obs, out):
    from aprilslam_amd.mapping import MapResult
    return [(f, s) for f, s, _, _ in MapResult(*out[:4], slot_weight=out[4], slot_ids=obs["id"]).soft_slots()]


# ---- the small and edge shapes of the device comparison: name -> (obs, dist, max_iters), each with one slipped corner
def keep_counts(obs, counts):
    """obs with only the first counts[f] slots of frame f left (none beyond len(counts))"""
    out = obs.copy()
    for f in range(out.shape[0]):
        k = 0
        for s in range(out.shape[1]):
            if out["id"][f, s] >= 0:
                k += 1
                if f >= len(counts) or k > counts[f]:
                    out["id"][f, s], out["flags"][f, s] = -1, 0
    return out


def empty_frames(n, max_tags):
    from aprilslam_amd._lib import OBS_DTYPE
    e = np.zeros((n, max_tags), dtype=OBS_DTYPE)
    e["id"] = -1
    return e


@functools.lru_cache(maxsize=None)
def edge_cases():
    cases = {}
    two, _, _ = noisy_block(2, 2)
    cases["2x2"] = (slip(two, 1, 0), None)
    four, _, _ = noisy_block(3, 4)
    for counts in ((3, 2), (4, 3), (4, 4), (4, 3, 2)):      # the linearisation takes four observations per workgroup
        cases["active_%d" % sum(counts)] = (slip(keep_counts(four, counts), 1, 1), None)
    wide, _, _ = noisy_block(14, 24)                        # 20 tags a frame; the fixed-order sums run 256 wide
    for n in (255, 256, 257):
        cases["active_%d" % n] = (slip(keep_counts(wide, [20] * 12 + [n - 240]), 6, 0), None)
    for mt in (2, 4, 24):
        b, _, _ = noisy_block(5, mt)
        cases["max_tags_%d" % mt] = (slip(b, 2, 1), None)
    six, _, _ = noisy_block(6, 8)
    six = slip(six, 3, 0)
    e = empty_frames(2, 8)
    cases["empty_first"] = (np.concatenate([e, six]), None)
    cases["empty_middle"] = (np.concatenate([six[:3], e, six[3:]]), None)
    cases["empty_last"] = (np.concatenate([six, e]), None)
    cases["behind"] = (behind_case(), None)
    return cases


def behind_case():
    """6 x 8 with a slipped corner and one observation the behind-camera test drops (weight 0).  The 1e12 of a corner behind
    the camera makes the sweeps take any candidate that has every corner in front, so the observation must be behind its
    camera under all of them: tag 7 keeps a single view, in frame 0, whose only other seeding slot is the world tag's, and
    its PnP translation t is chosen behind both the camera the world tag's pose implies and its mirrored planar minimum.
    With A the rotation between the two, t = t0 - c (e_z + A^T e_z) has z = t0_z - c (1 + A_zz) in both.  The tag's own
    candidates keep t, and the flip test has no row to move by."""
    six, _, _ = noisy_block(6, 8)
    out = slip(six, 3, 0)
    victim = sorted({int(i) for i in out["id"].ravel() if i >= 0})[-1]
    views = np.argwhere(out["id"] == victim)
    for f, s in views[1:]:
        out["id"][f, s], out["flags"][f, s] = -1, 0
    f0, s0 = views[0]
    assert f0 == 0 and out["id"][0, 0] == min(i for i in out["id"].ravel() if i >= 0)
    out["flags"][0, 1:s0] = 1
    T0 = MR.rec4(out["T"][0, 0])
    A = MR.mirror4(T0)[:3, :3] @ T0[:3, :3].T
    ez = np.array([0.0, 0.0, 1.0])
    assert 1.0 + A[2, 2] > 0.5
    T = MR.rec4(out["T"][f0, s0])
    T[:3, 3] = T0[:3, 3] - 4.0 * T0[2, 3] / (1.0 + A[2, 2]) * (ez + A.T @ ez)
    out["T"][f0, s0] = T[:3].ravel()
    return out


# Bound of the device against the statement, as smooth_cases.DEVICE_TOL: ten times the largest distance (LC.rel_err of every
# valid tag pose and every frame pose) between the statement and the statement with its sums over the observations
# reversed, over every compared case (the repair cases and the edge shapes, TAIL_CASES at COMPARE_ITERS trials), floor 1e-9.
# Measured: 2.545e-14, at one of TAIL_CASES; 6.77e-15 over the converged ones.
DEVICE_TOL_MEASURED = 2.545e-14
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)
# Cases whose trial count that perturbation changes (12 against 9, 7 against 8): the rounding of the tail decides it.  They
# are compared at COMPARE_ITERS trials from the seed; their converged results moved by the distance beside them, and the
# converged device result must lie within ten times that of the converged statement.
TAIL_CASES = {"active_8": 2.38e-12, "max_tags_2": 1.94e-12}


def distance(a, b):
    """largest LC.rel_err between two outputs' valid tag poses and frame poses"""
    assert np.array_equal(a[1]["valid"], b[1]["valid"])
    return max([LC.rel_err(MR.rec4(x), MR.rec4(y)) for x, y, v in zip(a[1]["T"], b[1]["T"], a[1]["valid"]) if v] +
               [LC.rel_err(x, y) for x, y in zip(a[3]["T"], b[3]["T"])])


def compared_cases():
    """(name, obs, dist, max_iters) of every case the device is compared on"""
    out = [(n, c[0], c[3], ITERS) for n, c in repair_cases().items()]
    out += [(n, c[0], c[1], COMPARE_ITERS if n in TAIL_CASES else ITERS) for n, c in edge_cases().items()]
    return out


def run(obs, dist, huber=HUBER, max_iters=ITERS, reverse=False, trace=None, with_std=True):
    return MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, huber_px=huber, max_iters=max_iters, trace=trace, reverse=reverse,
                         with_std=with_std)
