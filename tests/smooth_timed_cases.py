"""Inputs and recorded bounds of the tests of the sequence localisation with frame times (tests/test_smooth_timed_ref.py on the
CPU, tests/test_gpu_smooth_timed.py on the device): the cases of tests/smooth_cases.py and tests/smooth_seq_cases.py with a time
for every frame.  Every figure in recorded() and DEVICE_TOL was measured on the CPU with the NumPy statement
(tests/smooth_ref.py with times) -- never with the kernels; test_smooth_timed_ref.py measures them again and requires the recorded
figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import localize_cases as LC
import smooth_cases as SC
import smooth_ref as SR
import smooth_seq_cases as SQ

# Bound of the device's T against the statement's, built as smooth_cases.DEVICE_TOL is: ten times the largest rel_err between
# the statement and the statement with every frame's corner sums accumulated in reversed slot order over all_cases() of this
# file, floor 1e-9.  Measured: 8.73e-14 at shape(5, 4, 5); the one-tag cases 0 (one slot has no order to reverse).
DEVICE_TOL_MEASURED = 8.733e-14
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)

# the gap scene: smooth_cases.noise() (40 frames, 0.3 px noise) with the frames GAP dropped, the frame index as the time
GAP = (10, 30)
GAP_SIGMAS = (0.3, 0.002, 0.06)
GAP_NEAR = (8, 9, 30, 31)      # the four frames next to the gap, as frames of the 40

# the half-step grid: the first 12 frames of noise() at times that are multiples of 0.5, steps of 0.5, 1 and 1.5
HALF_STEPS = (1, 2, 1, 3, 2, 1, 1, 2, 3, 1, 2)


def recorded():
    """the statement's figures, rounded up to 4 significant digits
    marg_gap: the largest rel_err of T, over the kept frames of the gap scene, between the timed statement on the kept frames
      and the plain statement (smooth_ref) on all 40 frames with the gap emptied, both at MAX_ITERS.  marg_half: the same
      between the timed statement on the half-step grid and the plain one on the doubled grid (a frame every 0.5, the frames
      without one emptied) at both motion sigmas times sqrt(0.5).  The two sides are the same minimum; they agree as far as
      two LM runs that stop on a 1e-12 decrease do.  The tests' bound is ten times these.
    pose_at_rel / pose_at_pos: pose_at of the timed solve at the dropped frames' times against the emptied-frames solve's
      poses of those frames: the largest rel_err of T / position difference (scene units).  First order in the step
      rotation, so not rounding: the tests' bound is twice these.
    cov_scaled: the timed statement's covariance at the kept frames against the emptied-frames statement's, the largest
      |difference| / (std_i std_j).  Twice this is the tests' bound.
    gap_*: position RMSE against the truth (scene units) of the timed call and of the naive one (the plain call on the 20
      kept frames, one frame step across the gap), over GAP_NEAR and over all kept frames; gap_frame_near: of the
      per-frame localisation over GAP_NEAR."""
    return {"marg_gap": 9.218e-10, "marg_half": 2.567e-8, "pose_at_rel": 7.795e-4, "pose_at_pos": 1.419e-3, "cov_scaled": 8.415e-4,
            "gap_timed_near": 0.1330, "gap_naive_near": 0.2596, "gap_timed_all": 0.1200, "gap_naive_all": 0.1793,
            "gap_frame_near": 0.4993}


def times_of(n, key):
    """irregular frame times: cumsum(uniform(0.25, 4)), seeded by `key`"""
    return np.cumsum(np.random.default_rng(key).uniform(0.25, 4.0, n))


@functools.lru_cache(maxsize=None)
def shape_times(n, max_tags, n_dist):
    return times_of(n, 7000 + 100 * n + 10 * max_tags + n_dist)


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(name, obs, map records, seeds, dist, times, sigmas, max_iters)]: SC.SHAPES and SC.edge_sequences() with irregular times,
    COMPARE_ITERS trials.  n = 1 has no pair, n = 2 one; 64 / 65 / 130 cross the 64-frame loads of the scan and the dynamic
    programme; hole70's posed predecessor is more than a wavefront back, so the chain divides by a time difference across
    chunks"""
    out = [("shape%d_%d_%d" % s,) + SC.shape(*s) + (shape_times(*s), SC.SHAPE_SIGMAS, SC.COMPARE_ITERS) for s in SC.SHAPES]
    for k, (name, (obs, rec, seed)) in enumerate(SC.edge_sequences().items()):
        out.append((name, obs, rec, seed, None, times_of(len(obs), 9000 + k), SC.SHAPE_SIGMAS, SC.COMPARE_ITERS))
    return out


def case(name):
    return [c for c in all_cases() if c[0] == name][0][1:]


def run(obs, rec, seed, dist, times, sigmas, reverse=False, max_iters=SC.MAX_ITERS, huber=0.0):
    return SR.smooth(obs, rec, SC.K, dist, SC.TAG, seed, *sigmas, max_iters, reverse=reverse, huber_px=huber, times=times)


@functools.lru_cache(maxsize=None)
def statement(name):
    """the timed statement's (poses, result, trace) of a case of all_cases(), computed once"""
    obs, rec, seed, dist, times, sig, iters = case(name)
    return run(obs, rec, seed, dist, times, sig, max_iters=iters)


@functools.lru_cache(maxsize=None)
def ragged(max_tags=4):
    """(smooth_seq_cases.ragged(max_tags), times): every sequence with shape_times of its own, which start again near 0, so
    the times go backwards at each boundary"""
    b = SQ.ragged(max_tags)
    return b, np.concatenate([shape_times(n, max_tags, 0) for n in SQ.RAGGED_LENGTHS])


BAD_STATUS = [0, 4, 4, 4]


@functools.lru_cache(maxsize=None)
def bad_times_batch():
    """(batch, times): shape(5, 4, 0) four times over: good times, one NaN time, two equal times, one decreasing pair"""
    obs, rec, seed, _ = SC.shape(5, 4, 0)
    b = SQ.join([(obs, seed)] * 4, rec, None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)
    t = np.tile(shape_times(5, 4, 0), (4, 1))
    t[1, 2] = np.nan
    t[2, 3] = t[2, 2]
    t[3, 4] = t[3, 3] - 0.5
    return b, t.ravel()


def kept_frames():
    return np.array([f for f in range(40) if not GAP[0] <= f < GAP[1]])


@functools.lru_cache(maxsize=None)
def gap_scene():
    """(obs, map records, seeds, truths) of noise(), all 40 frames; the kept frames are kept_frames(), their times the frame
    indices"""
    return SC.noise()


@functools.lru_cache(maxsize=None)
def gap_statements():
    """(timed on the kept frames, naive: the plain statement on the kept frames, emptied: the plain statement on all 40 frames
    with the gap emptied and unseeded), each (poses, result, trace) at MAX_ITERS"""
    obs, rec, seed, _ = gap_scene()
    k = kept_frames()
    timed = run(obs[k], rec, seed[k], None, k.astype(np.float64), GAP_SIGMAS)
    naive = SC.run(obs[k], rec, seed[k], None, GAP_SIGMAS)
    return timed, naive, SC.run(*emptied_gap(), None, GAP_SIGMAS)


def emptied_gap():
    """(obs, map records, seeds) of the 40 frames with the gap emptied: the seeds of the per-frame localisation of that block"""
    obs, rec, _, _ = gap_scene()
    e = SC.empty(obs, range(*GAP))
    return e, rec, SC.seeds_of(e, rec)


def rmse(T, truth, frames=None):
    e = SC.pos_err(T, truth)
    return float(np.sqrt(np.mean((e if frames is None else e[list(frames)]) ** 2)))


def gap_rmses(timed_T, naive_T):
    """{gap_timed_near, gap_naive_near, gap_timed_all, gap_naive_all, gap_frame_near} of poses of the kept frames"""
    _, _, seed, truth = gap_scene()
    k = kept_frames()
    near = [int(np.flatnonzero(k == f)[0]) for f in GAP_NEAR]
    return {"gap_timed_near": rmse(timed_T, truth[k], near), "gap_naive_near": rmse(naive_T, truth[k], near),
            "gap_timed_all": rmse(timed_T, truth[k]), "gap_naive_all": rmse(naive_T, truth[k]),
            "gap_frame_near": rmse(seed["T"][k], truth[k], near)}


@functools.lru_cache(maxsize=None)
def half_grid():
    """((obs, map records, seeds, times) of the timed side, (obs, map records, seeds, grid indices) of the doubled grid):
    noise()'s first 12 frames at times 0.5 * cumsum(HALF_STEPS); the doubled grid has a frame every 0.5, empty where the timed
    side has none"""
    obs, rec, seed, _ = SC.noise()
    n = len(HALF_STEPS) + 1
    g = np.concatenate([[0], np.cumsum(HALF_STEPS)])
    wide = SC.empty(np.repeat(obs[:1], g[-1] + 1, axis=0), range(g[-1] + 1))
    wide[g] = obs[:n]
    return (obs[:n], rec, seed[:n], 0.5 * g), (wide, rec, SC.seeds_of(wide, rec), g)


def worst_rel(Ta, Tb):
    return max(LC.rel_err(a, b) for a, b in zip(Ta, Tb))


def scaled_cov_err(got, want):
    """the largest |got - want| / (std_i std_j) over (n, 6, 6) covariances"""
    worst = 0.0
    for g, w in zip(got, want):
        s = np.sqrt(np.diag(w))
        worst = max(worst, float((np.abs(g - w) / np.outer(s, s)).max()))
    return worst
