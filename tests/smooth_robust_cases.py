"""Inputs and recorded figures of the robust sequence-localisation tests (tests/test_smooth_robust_ref.py on the CPU,
tests/test_gpu_smooth_robust.py on the device).  Every figure in recorded() and ROBUST_TOL was measured on the CPU with the
NumPy statement (tests/smooth_ref.py at huber_px > 0) -- never with the kernels; test_smooth_robust_ref.py measures them again and
requires the recorded figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import smooth_cases as SC
import smooth_seq_cases as SQ

SHAPE_HUBER = 0.6
SHAPE_MOVE = (8.0, -6.0)            # pixels: corner 0 of slot 0 of every third frame
SHAPES = [(n, mt, nd) for n in (1, 2, 3, 5, 65) for mt in (1, 4, 20) for nd in ((0, 5) if n == 5 else (0,))]

SCENE_HUBER = 0.9
SCENE_ITERS = 30
# noise() corrupted in five of its 160 slots.  (frame, slot, corner, (du, dv)): one corner moved by 8 to 11 px
SCENE_MOVED = ((5, 0, 1, (6.0, -5.5)), (17, 2, 3, (-9.0, 4.0)), (29, 3, 0, (7.0, 8.4)))
# (frame, slot, slot of the same frame whose corners it holds): a wrong id, or a duplicate that survived de-duplication
SCENE_SWAPPED = ((11, 1, 3), (34, 0, 2))
SCENE_FRAMES = sorted([m[0] for m in SCENE_MOVED] + [s[0] for s in SCENE_SWAPPED])

# Bound of the device's T against the statement's: ten times the largest rel_err of T between the statement and the statement
# with every frame's corner sums in reversed slot order (a pure rounding perturbation) over the shapes, the scene and the
# two batches of this file, floor 1e-9: the rule smooth_cases.DEVICE_TOL follows.  Measured: 4.15e-14 at shape(5, 4, 0) (the
# scene, at its 30 trials, 3.08e-14 with the same trials and soft slots either way; the one-tag cases 0, one slot having no
# order to reverse).
ROBUST_TOL_MEASURED = 4.150e-14
ROBUST_TOL = max(10 * ROBUST_TOL_MEASURED, 1e-9)


def recorded():
    """the statements' figures on the scene, position RMSE against the truth in scene units, rounded up to 4 significant digits
    scene_rmse_seed: the per-frame localisation of the corrupted block (the seeds; two of them are hundreds of units off)
    scene_rmse_plain: smooth_ref on the corrupted block from those seeds at SCENE_ITERS trials, rounded DOWN (a lower bound)
    scene_rmse_robust: smooth_ref at SCENE_HUBER from the same seeds (largest single error 1.09)
    clean_rmse_robust: smooth_ref at SCENE_HUBER on the uncorrupted noise(); the plain problem gives 0.1380683 there, this
      0.1380686 (one slot of 160 is soft)
    scene_trials / scene_soft: the robust statement's trials (all of SCENE_ITERS: the linear tail converges slowly; the clean
      run stops after 5) and n_soft on the scene: 10 soft slots in the frames 5, 11, 17, 29, 32, 34, 35 -- the five corrupted
      slots, the slots a swapped one drags along in its frame, and two slots of plain noise over 0.9 px"""
    return {"scene_rmse_seed": 66.22, "scene_rmse_plain": 39.97, "scene_rmse_robust": 0.2390, "clean_rmse_robust": 0.1381,
            "scene_trials": 30, "scene_soft": 10}


def moved(obs, frame, slot, corner, d):
    out = obs.copy()
    c = out["corners"][frame, slot].astype(np.float64).reshape(4, 2)
    c[corner] += d
    out["corners"][frame, slot] = c.ravel().astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def shape(n, max_tags, n_dist):
    """(obs, map records, seeds, dist): smooth_cases.shape(n, max_tags, n_dist) -- the bench trajectory at 520 frames a round,
    0.2 px noise, seeds from the noise-free corners, every 7th frame emptied for n >= 5 -- with corner 0 of slot 0 of every
    third frame moved by SHAPE_MOVE.  With 20 slots a frame has 80 corners: a lane holds two, and the slot's OR over its
    corners runs in the second round as well."""
    obs, rec, seed, dist = SC.shape(n, max_tags, n_dist)
    for f in range(0, n, 3):
        obs = moved(obs, f, 0, 0, SHAPE_MOVE)
    return obs, rec, seed, dist


@functools.lru_cache(maxsize=None)
def scene(corrupt=True):
    """(obs, map records, seeds, truths): smooth_cases.noise() with the five slots of SCENE_MOVED and SCENE_SWAPPED corrupted,
    seeded by the per-frame localisation of the corrupted block (corrupt False: noise() itself)"""
    obs, rec, seed, truth = SC.noise()
    if not corrupt:
        return obs, rec, seed, truth
    obs = obs.copy()
    for f, s, c, d in SCENE_MOVED:
        obs = moved(obs, f, s, c, d)
    src = obs.copy()
    for f, s, other in SCENE_SWAPPED:
        obs["corners"][f, s] = src["corners"][f, other]
    return obs, rec, SC.seeds_of(obs, rec), truth


@functools.lru_cache(maxsize=None)
def ragged():
    """shape(n, 4, 0) for n in 1, 2, 3, 5, 65 end to end: 76 frames, 5 sequences"""
    cases = [shape(n, 4, 0) for n in (1, 2, 3, 5, 65)]
    return SQ.join([(c[0], c[2]) for c in cases], cases[0][1], None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS, SHAPE_HUBER)


MIXED_STATUS = [0, 0, 2, 3]
MIXED_COV_STATUS = [0, 0, 1, 1]


@functools.lru_cache(maxsize=None)
def mixed():
    """a clean sequence (smooth_cases.shape(5, 4, 0)), the same with its outliers (shape(5, 4, 0)) and the inputs of
    smooth_cases.failure_cases() (behind: never positive definite; nonfinite: no trial): result statuses MIXED_STATUS"""
    clean, dirty, fc = SC.shape(5, 4, 0), shape(5, 4, 0), SC.failure_cases()
    parts = [(clean[0], clean[2]), (dirty[0], dirty[2]), (fc["behind"][0], fc["behind"][2]), (fc["nonfinite"][0], fc["nonfinite"][2])]
    return SQ.join(parts, clean[1], None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS, SHAPE_HUBER)


def run(obs, rec, seed, dist, sigmas, huber, max_iters, reverse=False):
    return SC.run(obs, rec, seed, dist, sigmas, reverse, max_iters, huber)


def all_cases():
    """[(name, obs, map records, seeds, dist, sigmas, huber_px, max_iters)]: the shapes and the scene"""
    out = [("shape%d_%d_%d" % s,) + shape(*s) + (SC.SHAPE_SIGMAS, SHAPE_HUBER, SC.COMPARE_ITERS) for s in SHAPES]
    out.append(("scene",) + scene()[:3] + (None, SC.NOISE_SIGMAS, SCENE_HUBER, SCENE_ITERS))
    return out


@functools.lru_cache(maxsize=None)
def statement(name):
    """the robust statement's (poses, result, trace) of a case of all_cases(), computed once"""
    _, obs, rec, seed, dist, sig, huber, iters = [c for c in all_cases() if c[0] == name][0]
    return run(obs, rec, seed, dist, sig, huber, iters)


@functools.lru_cache(maxsize=None)
def batch_statement(which, k):
    """the robust statement's (poses, result, trace) of sequence k of ragged() / mixed() alone"""
    return SQ.statement(ragged() if which == "ragged" else mixed(), k)


def rmse(T, truth):
    return float(np.sqrt(np.mean(SC.pos_err(T, truth) ** 2)))


def up4(x):
    """x rounded up to 4 significant digits, as smooth_cases.recorded() holds its figures"""
    if x == 0:
        return 0.0
    e = 10.0 ** (np.floor(np.log10(abs(x))) - 3)
    return float("%.4g" % (np.ceil(x / e) * e))
