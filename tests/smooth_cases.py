"""Inputs and recorded bounds of the sequence-localisation tests (tests/test_smooth_ref.py on the CPU,
tests/test_gpu_smooth.py on the device).  Every figure in recorded() and DEVICE_TOL was measured on the CPU with the NumPy
statement (tests/smooth_ref.py) -- never with the kernels; test_smooth_ref.py measures them again and requires the recorded
figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import smooth_ref as SR
from aprilslam_amd import synth
from aprilslam_amd.localize import TagMap

K = synth.camera_matrix(LC.W, LC.H, 45.0)
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
TAG = LC.TAG_INNER
MAX_ITERS = 30
# The trials of the device-against-statement comparison (shape(), edge_sequences()).  The LM ends on an accepted trial whose
# decrease is below 1e-12 of the cost; at a converged pose the sign of a trial's decrease is decided by rounding, so the number
# of trials in that tail is not a property of the input: the statement itself, run with reversed corner sums, takes 11 trials
# where it took 6 (shape(65, 4, 5) at 30 trials), 7 for 6 at the 70-frame hole, and its poses then move by up to 3.3e-8.
# Three trials from seeds that are not yet the optimum are all in the steep part, where every accept / reject decision has a
# margin far above rounding: there the comparison is of the arithmetic, trial by trial.  The converged runs are the scenes
# (holes, flips, noise) at MAX_ITERS.
COMPARE_ITERS = 3

# Bound of the device's T against the statement's: ten times the largest rel_err between the statement and the statement
# with every frame's corner sums accumulated in reversed slot order (a pure rounding perturbation) over all the cases of
# this file, floor 1e-9.  Measured: 4.97e-14 at shape(3, 4, 0), the one-tag cases 0 (one slot has no order to reverse).
DEVICE_TOL_MEASURED = 4.971e-14
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)

# the scenes' priors: corner sigma in pixels, rotation in radians and translation in scene units per frame step
HOLES_SIGMAS = (0.05, 0.05, 2.0)
FLIPS_SIGMAS = (0.02, 0.05, 2.0)
NOISE_SIGMAS = (0.3, 0.004, 0.12)
NOISE_SEED, NOISE_PX = 7, 0.3


def recorded():
    """the statement's figures, rounded up to 4 significant digits
    holes_end_err / holes_mid_err: position error against the truth of the emptied frames 0 and 6 / of frame 3 of holes()
      (scene units).  A random walk holds an end frame at its neighbour, one frame step (0.3 units) from the truth, and
      puts frame 3 half way between its neighbours, where the straight trajectory has it.
    flips_margin / flips_first_margin: the largest final rotation error of the re-mirrored frames of flips() /
      flips(first=True) over the largest rotation error of the unmirrored frames' seeds (1.9e-5 rad: float32 corners of a
      tag of 40 pixels).  The mirrored seeds are 0.05 to 0.07 rad off; what is left is the prior's pull on a frame whose one
      small tag holds its rotation weakly, largest at the end of the sequence.
    noise_rmse_frame / noise_rmse_smooth: position RMSE against the truth of the per-frame localisation / of the statement
      on noise() (scene units)."""
    return {"holes_end_err": 0.3001, "holes_mid_err": 1.409e-5, "flips_margin": 10.59, "flips_first_margin": 77.10,
            "noise_rmse_frame": 0.4276, "noise_rmse_smooth": 0.1381}


def seeds_of(obs, rec, dist=None):
    """the per-frame localisation of the block: what asl_localize_frames_device writes for it"""
    return LR.localize(obs, rec, K, dist, TAG)


def empty(obs, frames):
    out = obs.copy()
    for f in frames:
        out["flags"][f] = 0
        out["id"][f] = -1
    return out


def mirror_seed(pb, seed, frames):
    """the seeds of `frames` replaced by their mirrored planar minima (candidate B of the chain)"""
    out = seed.copy()
    cand = SR.candidates(pb, seed)
    for f in frames:
        R, t = cand[f][1]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
        out["T"][f] = T
    return out


def truths(cams):
    return np.array([LC.world_from_camera(p, r) for p, r in cams])


@functools.lru_cache(maxsize=None)
def holes():
    """(obs, map records, seeds, truths): exact corners on a straight, rotation-free trajectory of 7 frames, 4 tags, frames
    0, 3 and 6 emptied"""
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    cams = [((-0.9 + 0.3 * i, 0.2, 0.5), (0.0, 0.0, 0.0)) for i in range(7)]
    obs = empty(np.stack([LC.exact_frame(tags, p, r, K, max_tags=4) for p, r in cams]), (0, 3, 6))
    return obs, rec, seeds_of(obs, rec), truths(cams)


FLIP_TAG = [{"id": 0, "position": [2.0, -1.0, -160.0], "rotation": [0.0, 0.0, 0.0]}]


@functools.lru_cache(maxsize=None)
def flips(first=False):
    """(obs, map records, seeds, truths, mirrored frames): 12 frames of one small, near-frontal tag (max_tags 1), the seeds
    of frames 3, 4 and 9 (first: of frame 0) replaced by their mirrored minima"""
    rec = TagMap.from_scene(FLIP_TAG).as_records()
    cams = [((-3.0 + 0.5 * i, 1.0 + 0.2 * i, 0.3 * i), (2.0 + 0.1 * i, -3.0 + 0.15 * i, 0.2 * i)) for i in range(12)]
    obs = np.stack([LC.exact_frame(FLIP_TAG, p, r, K, max_tags=1) for p, r in cams])
    seed = seeds_of(obs, rec)
    frames = (0,) if first else (3, 4, 9)
    pb = SR.problem(obs, rec, K, None, TAG, *FLIPS_SIGMAS)
    return obs, rec, mirror_seed(pb, seed, frames), truths(cams), frames


def noisy(obs, px, seed):
    out = obs.copy()
    rng = np.random.default_rng(seed)
    noise = rng.normal(0.0, px, out["corners"].shape)
    out["corners"] = (out["corners"].astype(np.float64) + noise).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def noise():
    """(obs, map records, seeds, truths): 40 consecutive frames of the bench trajectory at 400 frames a round, 4 tags, float32
    corners plus Gaussian noise of NOISE_PX from NOISE_SEED"""
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    cams = LC.trajectory(400)[:40]
    obs = noisy(np.stack([LC.exact_frame(tags, p, r, K, max_tags=4) for p, r in cams]), NOISE_PX, NOISE_SEED)
    return obs, rec, seeds_of(obs, rec), truths(cams)


SHAPES = [(n, mt, nd) for n in (1, 2, 3, 5, 64, 65, 130) for mt in (1, 4) for nd in ((0, 5) if n in (5, 65) else (0,))]
SHAPE_SIGMAS = (0.5, 0.01, 0.2)


@functools.lru_cache(maxsize=None)
def shape(n, max_tags, n_dist):
    """(obs, map records, seeds, dist) of the device-against-statement comparison: n consecutive frames of the bench
    trajectory at 520 frames a round, corners with 0.2 px noise, seeded by the localisation of the same frames without the
    noise (so that the first trials have work to do); every 7th frame from the 4th on emptied (n >= 5), and with one tag a
    frame the seeds of frames 1 and n - 3 mirrored (n >= 5)"""
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    dist = DIST5 if n_dist else None
    cams = LC.trajectory(520)[:n]
    exact = np.stack([LC.exact_frame(tags, p, r, K, dist=dist, max_tags=max_tags) for p, r in cams])
    obs = noisy(exact, 0.2, 100 * n + max_tags)
    if n >= 5:
        obs, exact = empty(obs, range(3, n, 7)), empty(exact, range(3, n, 7))
    seed = seeds_of(exact, rec, dist)
    if max_tags == 1 and n >= 5:
        seed = mirror_seed(SR.problem(obs, rec, K, dist, TAG, *SHAPE_SIGMAS), seed, (1, n - 3))
    return obs, rec, seed, dist


def edge_sequences():
    """{name: (obs, map records, seeds)}: all frames empty; only the first / only the last frame posed; a hole of 70 frames;
    max_tags 1 with n_ids 1"""
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    cams = LC.trajectory(520)[:75]
    full = np.stack([LC.exact_frame(tags, p, r, K, max_tags=4) for p, r in cams])
    out = {}
    for name, obs in (("all_empty", empty(full[:6], range(6))), ("first_only", empty(full[:6], range(1, 6))),
                      ("last_only", empty(full[:6], range(5))), ("hole70", empty(full, range(2, 72)))):
        out[name] = (obs, rec, seeds_of(obs, rec))
    rec1 = TagMap.from_scene(FLIP_TAG).as_records()
    obs1 = flips()[0][:5]
    out["one_id"] = (obs1, rec1, LR.localize(obs1, rec1, K, None, TAG))
    return out


def failure_cases():
    """{name: (obs, map records, seeds, sigmas, max_iters, result status, trials)}: solves that cannot succeed
    behind: one frame of 4 tags whose seed looks the other way (world<-camera turned half round about its x axis): every
      corner is behind the camera, H and g are zero, so the one diagonal block is never positive definite: result status 2,
      every trial run and failed, T the seed's
    nonfinite: two frames, the second's seed pose NaN: the motion cost after the chain is not finite: status 3, no trial"""
    obs, rec, seed, _ = holes()
    behind = seed[1:2].copy()
    behind["T"][0] = behind["T"][0] @ np.diag([1.0, -1.0, -1.0, 1.0])
    nonfinite = seed[1:3].copy()
    nonfinite["T"][1] = np.nan
    return {"behind": (obs[1:2], rec, behind, HOLES_SIGMAS, 4, SR.NOT_POSITIVE_DEFINITE, 4),
            "nonfinite": (obs[1:3], rec, nonfinite, HOLES_SIGMAS, 4, SR.NON_FINITE, 0)}


def run(obs, rec, seed, dist, sigmas, reverse=False, max_iters=MAX_ITERS, huber=0.0):
    return SR.smooth(obs, rec, K, dist, TAG, seed, *sigmas, max_iters, reverse=reverse, huber_px=huber)


def pos_err(T, truth):
    return np.linalg.norm(np.asarray(T)[..., :3, 3] - np.asarray(truth)[..., :3, 3], axis=-1)


def chain_margin(trace):
    """the least relative amount by which toggling one posed frame's choice raises the chain cost (inf without a choice)"""
    d, tr, choice = trace["d"], trace["tr"], trace["choice"]
    base = SR.chain_total(d, tr, choice)
    worst = np.inf
    for k in range(len(choice)):
        if d[k, 0] == d[k, 1] and np.array_equal(tr[k, :, 0], tr[k, :, 1]):
            continue    # B = A
        alt = choice.copy()
        alt[k] ^= 1
        worst = min(worst, (SR.chain_total(d, tr, alt) - base) / max(1.0, base))
    return worst


def all_cases():
    """[(name, obs, map records, seeds, dist, sigmas, max_iters)]: every case of this file"""
    out = [("holes",) + holes()[:3] + (None, HOLES_SIGMAS, MAX_ITERS), ("flips",) + flips()[:3] + (None, FLIPS_SIGMAS, MAX_ITERS),
           ("flips_first",) + flips(True)[:3] + (None, FLIPS_SIGMAS, MAX_ITERS), ("noise",) + noise()[:3] + (None, NOISE_SIGMAS, MAX_ITERS)]
    out += [("shape%d_%d_%d" % s,) + shape(*s) + (SHAPE_SIGMAS, COMPARE_ITERS) for s in SHAPES]
    out += [(k,) + v + (None, SHAPE_SIGMAS, COMPARE_ITERS) for k, v in edge_sequences().items()]
    return out


@functools.lru_cache(maxsize=None)
def statement(name):
    """the statement's (poses, result, trace) of a case of all_cases(), computed once"""
    _, obs, rec, seed, dist, sig, iters = [c for c in all_cases() if c[0] == name][0]
    return run(obs, rec, seed, dist, sig, max_iters=iters)


def flip_errors(T, first):
    """(largest rotation error of the re-mirrored frames of T, largest of the unmirrored frames' seeds)"""
    _, _, seed, tr, frames = flips(first)
    rest = [f for f in range(len(tr)) if f not in frames]
    return (max(LC.rot_err(T[f], tr[f]) for f in frames), max(LC.rot_err(seed["T"][f], tr[f]) for f in rest))
