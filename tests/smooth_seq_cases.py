"""Batches of sequences for asl_smooth_sequences_* (tests/test_smooth_seq_abi.py on the CPU, tests/test_gpu_smooth_sequences.py
on the device), built from the cases of tests/smooth_cases.py.  The statement of a batch is the statement of each of its
sequences alone (tests/smooth_ref.py, tests/smooth_cov_ref.py): nothing here states a batch of its own.  All batches share one
map (the bench scene), smooth_cases.K and one set of sigmas."""
import collections
import functools

import numpy as np

import smooth_cases as SC

Batch = collections.namedtuple("Batch", "obs rec seed dist seq_start sigmas max_iters huber")    # huber: 0 for the plain batches

RAGGED_LENGTHS = (1, 2, 3, 5, 64, 65, 130)
STOP_APART_CUTS = ((0, 40), (13, 14), (5, 7), (0, 13), (14, 40))
# the statement's trial counts of noise() cut as STOP_APART_CUTS that do not hang on a rounding (measured with smooth_ref, with
# the corner sums in either order): cut -> trials
STOP_APART_TRIALS = {(0, 40): 5, (5, 7): 5, (13, 14): 9}
FAILURES_TRIALS = 4
FAILURES_STATUS = [0, 2, 1, 3, 0]
FAILURES_COV_STATUS = [0, 1, 1, 1, 0]
SHORT_PATTERN = (1, 2, 3, 5)


def join(parts, rec, dist, sigmas, max_iters, huber=0.0):
    """parts: [(obs, seed)] of one max_tags -> the sequences laid end to end"""
    start = np.concatenate([[0], np.cumsum([len(o) for o, _ in parts])]).astype(np.int32)
    return Batch(np.concatenate([o for o, _ in parts]), rec, np.concatenate([s for _, s in parts]), dist, start, sigmas, max_iters, huber)


def ranges(batch):
    return [(int(a), int(b)) for a, b in zip(batch.seq_start[:-1], batch.seq_start[1:])]


@functools.lru_cache(maxsize=None)
def ragged(max_tags):
    """shape(n, max_tags, 0) for every n of RAGGED_LENGTHS: 270 frames, 7 sequences; with one tag a frame the seeds of the
    sequences of 5 frames and more include mirrored ones"""
    cases = [SC.shape(n, max_tags, 0) for n in RAGGED_LENGTHS]
    return join([(c[0], c[2]) for c in cases], cases[0][1], None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)


@functools.lru_cache(maxsize=None)
def ragged_dist():
    """shape(5, 4, 5) + shape(65, 4, 5): the five lens coefficients"""
    cases = [SC.shape(5, 4, 5), SC.shape(65, 4, 5)]
    return join([(c[0], c[2]) for c in cases], cases[0][1], cases[0][3], SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)


def ragged_names(batch_name):
    """the smooth_cases.all_cases() name of every sequence of a ragged batch"""
    if batch_name == "dist":
        return ["shape5_4_5", "shape65_4_5"]
    return ["shape%d_%d_0" % (n, int(batch_name)) for n in RAGGED_LENGTHS]


@functools.lru_cache(maxsize=None)
def stop_apart():
    """noise() cut as STOP_APART_CUTS: sequences that stop after different numbers of trials"""
    obs, rec, seed, _ = SC.noise()
    return join([(obs[a:b], seed[a:b]) for a, b in STOP_APART_CUTS], rec, None, SC.NOISE_SIGMAS, SC.MAX_ITERS)


@functools.lru_cache(maxsize=None)
def failures():
    """[holes(), behind, all_empty, nonfinite, holes()]: result statuses FAILURES_STATUS in FAILURES_TRIALS trials"""
    obs, rec, seed, _ = SC.holes()
    fc, es = SC.failure_cases(), SC.edge_sequences()
    parts = [(obs, seed), (fc["behind"][0], fc["behind"][2]), (es["all_empty"][0], es["all_empty"][2]),
             (fc["nonfinite"][0], fc["nonfinite"][2]), (obs, seed)]
    return join(parts, rec, None, SC.HOLES_SIGMAS, FAILURES_TRIALS)


def cut(lengths):
    """shape(130, 4, 0) cut into consecutive sequences of the given lengths (cycled until the frames run out)"""
    obs, rec, seed, _ = SC.shape(130, 4, 0)
    parts, a, k = [], 0, 0
    while a < len(obs):
        b = min(a + lengths[k % len(lengths)], len(obs))
        parts.append((obs[a:b], seed[a:b]))
        a, k = b, k + 1
    return parts, rec


@functools.lru_cache(maxsize=None)
def many_short():
    """130 sequences of one frame, three times over: 390 sequences, more workgroups than the device has CUs"""
    parts, rec = cut((1,))
    return join(parts * 3, rec, None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)


SEQ_CHUNK = 896   # sequences whose offsets one launch carries to the device (k_smooth.inc: SM_SEQ_CHUNK)


@functools.lru_cache(maxsize=None)
def past_one_chunk(n_seq):
    """the 130 one-frame sequences repeated until there are n_seq of them: at SEQ_CHUNK the offsets fill one launch exactly,
    at SEQ_CHUNK + 1 the last sequence is alone in a second launch, 910 is seven whole repeats"""
    parts, rec = cut((1,))
    return join((parts * (n_seq // len(parts) + 1))[:n_seq], rec, None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)


@functools.lru_cache(maxsize=None)
def short_pattern():
    """the same 130 frames cut 1, 2, 3, 5, 1, 2, 3, 5, ..."""
    parts, rec = cut(SHORT_PATTERN)
    return join(parts, rec, None, SC.SHAPE_SIGMAS, SC.COMPARE_ITERS)


def statement(batch, k):
    """the statement's (poses, result, trace) of sequence k of a batch alone"""
    a, b = ranges(batch)[k]
    return SC.run(batch.obs[a:b], batch.rec, batch.seed[a:b], batch.dist, batch.sigmas, max_iters=batch.max_iters, huber=batch.huber)
