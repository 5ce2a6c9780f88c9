"""Seeded inputs for the de-duplication stage (S8): shared by tests/test_dedup_ref.py (statement against the C oracle, on
the CPU) and tests/test_gpu_dedup.py (asl_debug_dedup against the statement).

A case is a Case(name, recs, keys, n_frames, cap): DET_DTYPE records with their frame index, one uint64 cluster key per
record (distinct within a frame in their low 48 bits; the high 16 carry noise, which the stage must ignore), the number
of frames and the per-frame list capacity of the call.  Quads are axis-aligned squares [lb, rb, rt, lt] unless a hand
case says otherwise; coordinates sit on a quarter-pixel grid, so touching and coinciding sides do occur."""
import itertools
from collections import namedtuple

import numpy as np

from aprilslam_amd._lib import DET_DTYPE

Case = namedtuple("Case", "name recs keys n_frames cap")

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)
FRAME_COUNTS = (1, 2, 64, 65, 1024, 1025, 2049)
_UNIT = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])


def records(ids, xy, size, hamming=0, margin=50.0, frame=0):
    """squares of side `size` with their lower-left corner at xy (n, 2)"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    r = np.zeros(len(xy), dtype=DET_DTYPE)
    r["id"], r["hamming"], r["margin"], r["frame"] = ids, hamming, margin, frame
    r["corners"] = xy[:, None, :] + np.asarray(size, dtype=np.float64).reshape(-1, 1, 1) * _UNIT
    r["center"] = r["corners"].mean(axis=1)
    return r


def quad(id_, corners, hamming=0, margin=50.0, center=None):
    r = np.zeros(1, dtype=DET_DTYPE)
    r["id"], r["hamming"], r["margin"] = id_, hamming, margin
    r["corners"] = np.asarray(corners, dtype=np.float64).reshape(4, 2)
    r["center"] = r["corners"].mean(axis=1) if center is None else center
    return r


def distinct_keys(rng, n):
    """n keys whose low 48 bits differ, in no order, with noise above bit 48"""
    low = (rng.choice(1 << 20, size=n, replace=False).astype(np.uint64) << np.uint64(28)) | rng.integers(0, 1 << 28, n).astype(np.uint64)
    return low | (rng.integers(0, 1 << 16, n).astype(np.uint64) << np.uint64(48))


def assemble(name, frames, cap, rng=None):
    """frames: a (recs, keys) pair per frame -> Case; rng: the records of all frames shuffled in memory, each with its key"""
    recs, keys = [], []
    for f, (r, k) in enumerate(frames):
        r = r.copy()
        r["frame"] = f
        recs.append(r)
        keys.append(np.asarray(k, dtype=np.uint64))
    recs, keys = np.concatenate(recs), np.concatenate(keys)
    if rng is not None:
        p = rng.permutation(len(recs))
        recs, keys = recs[p], keys[p]
    return Case(name, recs, keys, len(frames), cap)


# ---- hand cases: two or three records of one id per frame, keys ascending in memory order unless the label ends in _ba

def _sq(x, y, s):
    return [[x, y], [x + s, y], [x + s, y + s], [x, y + s]]


def hand_frames():
    """[(label, recs, keys)]: what survives each is written down in tests/test_dedup_ref.py"""
    ID = 7
    out = []

    def add(label, quads, keys=None):
        out.append((label, np.concatenate(quads), np.arange(1, len(quads) + 1, dtype=np.uint64) if keys is None else np.array(keys, dtype=np.uint64)))

    add("apart", [quad(ID, _sq(0, 0, 10)), quad(ID, _sq(30, 0, 10), margin=60)])
    add("shared_edge", [quad(ID, _sq(0, 0, 10)), quad(ID, _sq(10, 0, 10), margin=60)])
    add("shared_corner", [quad(ID, _sq(0, 0, 10)), quad(ID, _sq(10, 10, 10), margin=60)])
    add("half_pixel_apart", [quad(ID, _sq(0, 0, 10)), quad(ID, _sq(10.5, 0, 10), margin=60)])
    # nested: no sides cross, so only corner 0 of the inner quad, tested against the outer one, finds the overlap -- as the
    # second record it is the b[0]-in-a term, as the first the a[0]-in-b term
    add("nested_outer_first", [quad(ID, _sq(0, 0, 30)), quad(ID, _sq(10, 10, 5), margin=60)])
    add("nested_inner_first", [quad(ID, _sq(10, 10, 5), margin=60), quad(ID, _sq(0, 0, 30))])
    add("crossing", [quad(ID, [[0, 10], [30, 10], [30, 20], [0, 20]]), quad(ID, [[10, 0], [20, 0], [20, 30], [10, 30]], margin=60)])
    add("hamming_beats_margin", [quad(ID, _sq(0, 0, 10), hamming=0, margin=10), quad(ID, _sq(2, 2, 10), hamming=1, margin=90)])
    add("margin_beats_corners", [quad(ID, _sq(2, 2, 10), margin=50), quad(ID, _sq(0, 0, 10), margin=40)])
    base = np.array(_sq(0, 0, 10), dtype=np.float64).ravel()
    for k in range(8):  # equal up to coordinate k, smaller there, larger everywhere after it: only coordinate k can decide
        other = base.copy()
        other[k] += 0.25
        other[k + 1:] -= 0.125
        add("corner_tie_%d_ab" % k, [quad(ID, base), quad(ID, other)])
        add("corner_tie_%d_ba" % k, [quad(ID, base), quad(ID, other)], keys=[2, 1])
    add("identical_ab", [quad(ID, _sq(0, 0, 10), center=[1, 1]), quad(ID, _sq(0, 0, 10), center=[2, 2])])
    add("identical_ba", [quad(ID, _sq(0, 0, 10), center=[1, 1]), quad(ID, _sq(0, 0, 10), center=[2, 2])], keys=[2, 1])
    add("identical_three", [quad(ID, _sq(0, 0, 10), center=[c, c]) for c in (1, 2, 3)], keys=[2, 3, 1])
    add("two_of_three", [quad(ID, _sq(0, 0, 10)), quad(ID, _sq(5, 5, 10), margin=60), quad(ID, _sq(40, 0, 10), margin=40)])
    add("other_id_between", [quad(ID, _sq(0, 0, 10)), quad(ID + 1, _sq(1, 1, 10), margin=90), quad(ID, _sq(2, 2, 10), margin=60)])
    return out


CHAIN_MARGINS = tuple(itertools.permutations((90.0, 50.0, 40.0)))
CHAIN_KEYS = tuple(itertools.permutations((1, 2, 3)))


def chain_frames():
    """A - B - C along x: A overlaps B, B overlaps C, A and C are apart.  Every assignment of the three margins (the best
    record first, in the middle, last) under every order of the three keys: [(label, recs, keys)], label 'chain_m<i>_k<j>'
    for CHAIN_MARGINS[i] on (A, B, C) and CHAIN_KEYS[j] as their keys."""
    out = []
    for i, m in enumerate(CHAIN_MARGINS):
        for j, k in enumerate(CHAIN_KEYS):
            r = np.concatenate([quad(3, _sq(8 * a, 0, 10), margin=m[a]) for a in range(3)])
            out.append(("chain_m%d_k%d" % (i, j), r, np.array(k, dtype=np.uint64)))
    return out


def hand_case():
    frames = hand_frames() + chain_frames()
    return assemble("hand", [(r, k) for _, r, k in frames], cap=4), [label for label, _, _ in frames]


# ---- random material

def _mix(rng, n, ids, scale):
    """n squares of side 20 with ids drawn from `ids`, thrown into a field sized so that a record overlaps about
    1 / scale^2 others of its id; hamming 0..2, margins from eight values (ties leave the decision to the corners), one
    record in thirty an exact copy of another"""
    ids = np.asarray(ids)
    rid = ids[rng.integers(0, len(ids), n)]
    field = 40.0 * scale * np.sqrt(max(1.0, n / len(ids)))
    xy = np.round(rng.uniform(0, field, (n, 2)) * 4) / 4
    r = records(rid, xy, 20.0, hamming=rng.integers(0, 3, n), margin=rng.choice(np.arange(8) * 7.5 + 20, n))
    for dst in np.nonzero(rng.random(n) < 1 / 30)[0]:
        r[dst] = r[rng.integers(0, n)]
    return r


def size_case(n, kind):
    """kind 'distinct': n ids, a pure sort; 'mix': a few ids, eliminations all over the sorted list"""
    rng = np.random.default_rng(5000 + n * 2 + (kind == "mix"))
    if kind == "distinct":
        r = records(rng.permutation(2048)[:n], np.round(rng.uniform(0, 1000, (n, 2)) * 4) / 4, 20.0, hamming=rng.integers(0, 3, n),
                    margin=rng.uniform(20, 90, n).astype(np.float32))
    else:
        nids = (1, 2, 7, 50)[SIZES.index(n) % 4]
        r = _mix(rng, n, np.array([0, 1, 511] + list(range(2, 49)))[:nids], (0.5, 1.0, 2.0)[SIZES.index(n) % 3])
    return assemble("size_%d_%s" % (n, kind), [(r, distinct_keys(rng, n))], cap=1024)


def one_id_case(n, overlap):
    """n records of one id: all sharing a point (every test eliminates: linear), or none touching (n (n - 1) / 2 tests)"""
    rng = np.random.default_rng(7000 + n + overlap)
    if overlap:
        r = records(5, np.round(rng.uniform(0, 20, (n, 2)) * 4) / 4, 100.0, margin=rng.permutation(n).astype(np.float32))
    else:
        g = np.arange(n)
        r = records(5, np.stack([30.0 * (g % 32), 30.0 * (g // 32)], axis=1) + np.round(rng.uniform(0, 8, (n, 2)) * 4) / 4, 10.0,
                    hamming=rng.integers(0, 3, n), margin=rng.uniform(20, 90, n).astype(np.float32))
        r = r[rng.permutation(n)]
    return assemble("one_id_%d_%s" % (n, "all_overlap" if overlap else "none_overlap"), [(r, distinct_keys(rng, n))], cap=1024)


def _group(rng, id_, offsets, at):
    offsets = np.asarray(offsets, dtype=np.float64)
    xy = np.stack([at[0] + offsets, np.full(len(offsets), at[1])], axis=1)
    return records(id_, xy, 10.0, hamming=rng.integers(0, 2, len(offsets)), margin=rng.permutation(len(offsets)) * 5.0 + 30)


def _singles(ids):
    ids = np.asarray(ids)
    return records(ids, np.stack([40.0 * (ids % 32), 100.0 + 40.0 * (ids // 32)], axis=1), 10.0)


def placement_case():
    """Groups of one id at chosen positions of the sorted list (ids are the sort's major key): frame 0 a group at position 0
    and one ending at n - 1; frame 1 a group over positions 62..65 (lanes 63 / 64 of the first wavefront); frame 2 over
    254..257 (the two compaction chunks); frame 3 one record, a group of 300, one record.  Ids 0, 1 and 511 take part.  The
    groups of four are two overlapping pairs 30 px apart: two records die, one on each side of the boundary or both on one."""
    rng = np.random.default_rng(6100)
    pairs = [0.0, 6.0, 30.0, 36.0]
    f0 = np.concatenate([_group(rng, 0, [0.0, 5.0, 9.0], (0, 0)), _singles(np.arange(1, 41)), _group(rng, 511, [0.0, 5.0, 40.0], (0, 50))])
    f1 = np.concatenate([_singles(np.arange(0, 62)), _group(rng, 62, pairs, (0, 0)), _singles(np.arange(63, 101))])
    f2 = np.concatenate([_singles(np.arange(0, 254)), _group(rng, 254, pairs, (0, 0)), _singles(np.arange(255, 301))])
    big = _mix(rng, 300, [1], 1.0)
    f3 = np.concatenate([_singles([0]), big, _singles([511])])
    return assemble("placement", [(f, distinct_keys(rng, len(f))) for f in (f0, f1, f2, f3)], cap=512, rng=rng)


def limit_case():
    """three frames, the middle one with 1025 records: one more than the device sorts"""
    rng = np.random.default_rng(6200)
    f1 = records(np.arange(1025), np.round(rng.uniform(0, 1000, (1025, 2)) * 4) / 4, 20.0)
    frames = [_mix(rng, 40, [0, 1, 511], 1.0), f1, _mix(rng, 65, [3, 4], 1.0)]
    return assemble("limit_1025", [(f, distinct_keys(rng, len(f))) for f in frames], cap=2048, rng=rng)


def capacity_case(slack):
    """two frames of 300 and 17 records in lists of 300 + slack entries: slack 0 fits exactly, -1 overflows by one record"""
    rng = np.random.default_rng(6300)
    frames = [_mix(rng, 300, [0, 1, 2, 511], 1.0), _mix(rng, 17, [9], 1.0)]
    return assemble("capacity_%+d" % slack, [(f, distinct_keys(rng, len(f))) for f in frames], cap=300 + slack, rng=rng)


def frames_case(n_frames):
    """0 to 3 records per frame, of one id and close together, so that some are eliminated; the first, the middle and the last
    frame empty (from five frames on); the records of all frames interleaved in memory; lists of four entries"""
    rng = np.random.default_rng(6400 + n_frames)
    counts = rng.integers(0, 4, n_frames)
    if n_frames >= 5:
        counts[[0, n_frames // 2, n_frames - 1]] = 0
    elif n_frames == 2:
        counts[:] = (2, 0)
    else:
        counts[:] = 3
    frames = []
    for f, c in enumerate(counts):
        r = records(rng.integers(0, 2, c) * 511, np.round(rng.uniform(0, 25, (c, 2)) * 4) / 4, 10.0, hamming=rng.integers(0, 2, c),
                    margin=rng.choice([30.0, 60.0], c))
        frames.append((r, distinct_keys(rng, c)))
    return assemble("frames_%d" % n_frames, frames, cap=4, rng=rng)


def all_cases(one_id_none_overlap=1024):
    """every case both test files run; one_id_none_overlap: the size of the quadratic single-id group"""
    cases = [hand_case()[0], placement_case(), limit_case(), capacity_case(0), capacity_case(-1)]
    cases += [size_case(n, kind) for n in SIZES for kind in ("distinct", "mix")]
    cases += [one_id_case(1024, True), one_id_case(one_id_none_overlap, False)]
    cases += [frames_case(n) for n in FRAME_COUNTS]
    return cases
