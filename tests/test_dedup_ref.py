"""The de-duplication statement (tests/dedup_ref.py) against the C oracle's dedup_and_sort, byte for byte, on every case of
tests/dedup_cases.py, and the hand cases against answers written here.  Both are built without contraction and do the same
float64 operations, so there is no tolerance.  Also checks that the cases are what they claim to be (where the groups sit
in the sorted list, that records die in every 256-chunk) and that the oracle finds exactly the tags of the tag sheets."""
import numpy as np
import pytest

import dedup_cases as DC
import dedup_ref as R
import oracle_lib as O
import tag_sheet as TS

CASES = DC.all_cases()


def frame_of(case, f):
    m = case.recs["frame"] == f
    return case.recs[m], case.keys[m]


def sorted_alive(recs, keys):
    """the records in the device's sort order (id, key) and which of them the statement keeps"""
    k = keys & np.uint64(R.KEY_MASK)
    by_key = np.argsort(k)
    alive = R.eliminate(recs[by_key])
    order = np.lexsort((k[by_key], recs["id"][by_key]))
    return recs[by_key][order], alive[order]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_statement_equals_the_oracle(case):
    total = 0
    for f in range(case.n_frames):
        r, k = frame_of(case, f)
        mine = R.dedup_frame(r, k)
        ref = O.dedup_and_sort(r[np.argsort(k & np.uint64(R.KEY_MASK))])
        assert mine.tobytes() == ref.tobytes(), (case.name, f)
        total += len(mine)
    out, npf, cnt = R.dedup(case.recs, case.keys, case.n_frames, case.cap)
    assert len(out) == cnt[0] == npf.sum() and (cnt[1] or cnt[2] or cnt[0] == total)
    assert np.all(np.diff(out["frame"]) >= 0)


# label -> the records that stay, as indices into the frame's records in memory order, in output order
HAND = {
    "apart": [0, 1],
    "shared_edge": [1],          # corner 0 of the second lies on a side of the first: touching is overlap
    "shared_corner": [1],
    "half_pixel_apart": [0, 1],
    "nested_outer_first": [1],
    "nested_inner_first": [0],
    "crossing": [1],             # no corner of either inside the other: only the sides' crossing finds it
    "hamming_beats_margin": [0],
    "margin_beats_corners": [0],
    "identical_ab": [1],         # the later key stays
    "identical_ba": [0],
    "identical_three": [1],      # keys 2, 3, 1: the record with key 3
    "two_of_three": [1, 2],
    "other_id_between": [2, 1],  # ids 7, 8, 7: the 8 is not compared with anything; output by id
}
HAND.update({"corner_tie_%d_%s" % (k, o): [0] for k in range(8) for o in ("ab", "ba")})  # the smaller coordinate stays
# margins (A, B, C) under keys (A, B, C): B beats A and C beats B, so who meets whom first decides
CHAINS = {
    "chain_m5_k0": [2],      # margins 40 50 90, keys 1 2 3: A loses to B, B loses to C
    "chain_m5_k3": [0, 2],   # keys 2 3 1: C is walked first and removes B before A meets it
    "chain_m0_k0": [0, 2],   # margins 90 50 40, keys 1 2 3: A removes B, C meets nothing
    "chain_m0_k3": [0],      # keys 2 3 1: C walks first and loses to B, then A removes B
    "chain_m2_k0": [1],      # the best in the middle removes both, in any order
    "chain_m2_k5": [1],
}


def test_hand_cases_give_the_answers_written_here():
    case, labels = DC.hand_case()
    assert set(HAND) | set(CHAINS) <= set(labels) and len(set(labels)) == len(labels)
    for f, label in enumerate(labels):
        want = HAND.get(label, CHAINS.get(label))
        if want is None:
            continue
        r, k = frame_of(case, f)
        assert R.dedup_frame(r, k).tobytes() == r[want].tobytes(), label
    per_margins = {}
    for f, label in enumerate(labels):
        if label.startswith("chain_"):
            per_margins.setdefault(label[:8], set()).add(R.dedup_frame(*frame_of(case, f)).tobytes())
    assert len(per_margins) == 6 and sum(len(v) > 1 for v in per_margins.values()) >= 2, "no chain depends on the key order"


@pytest.mark.parametrize("n", DC.SIZES)
def test_size_cases_are_a_pure_sort_and_a_mix(n):
    d = DC.size_case(n, "distinct")
    assert len(np.unique(d.recs["id"])) == n == len(R.dedup_frame(d.recs, d.keys))
    assert np.any(np.diff(np.argsort(d.keys & np.uint64(R.KEY_MASK))) < 0) or n == 1, "keys follow the memory order"
    m = DC.size_case(n, "mix")
    _, alive = sorted_alive(m.recs, m.keys)
    if n >= 63:
        for start in range(0, n, 256):
            chunk = alive[start:start + 256]
            assert len(chunk) < 32 or (not chunk.all() and chunk.any()), (n, start)


def test_placement_case_puts_its_groups_where_it_says():
    case = DC.placement_case()

    def group_span(f, id_):
        s, alive = sorted_alive(*frame_of(case, f))
        at = np.nonzero(s["id"] == id_)[0]
        return int(at[0]), int(at[-1]), len(s), alive[at]

    lo, hi, n, alive = group_span(0, 0)
    assert lo == 0 and hi == 2 and not alive.all()
    lo, hi, n, alive = group_span(0, 511)
    assert hi == n - 1 and hi - lo == 2 and not alive.all() and alive.sum() == 2
    lo, hi, n, alive = group_span(1, 62)
    assert (lo, hi) == (62, 65) and alive.sum() == 2
    lo, hi, n, alive = group_span(2, 254)
    assert (lo, hi) == (254, 257) and alive.sum() == 2
    lo, hi, n, alive = group_span(3, 1)
    assert (lo, hi, n) == (1, 300, 302) and 0 < alive.sum() < 300


def test_limits_in_the_statement():
    c = DC.limit_case()
    assert np.bincount(c.recs["frame"]).tolist() == [40, 1025, 65]
    out, npf, cnt = R.dedup(c.recs, c.keys, c.n_frames, c.cap)
    assert npf[1] == 0 and npf[0] > 0 and npf[2] > 0 and cnt.tolist() == [npf.sum(), 0, 1]
    fits, over = DC.capacity_case(0), DC.capacity_case(-1)
    assert fits.recs.tobytes() == over.recs.tobytes() and np.bincount(fits.recs["frame"]).max() == fits.cap == over.cap + 1
    assert R.dedup(fits.recs, fits.keys, 2, fits.cap)[2].tolist()[1:] == [0, 0]
    out, npf, cnt = R.dedup(over.recs, over.keys, 2, over.cap)
    assert len(out) == 0 and not npf.any() and cnt[0] == 0 and cnt[1] > 0


@pytest.mark.parametrize("n_frames", DC.FRAME_COUNTS)
def test_frames_cases_have_their_empty_frames(n_frames):
    c = DC.frames_case(n_frames)
    per = np.bincount(c.recs["frame"], minlength=n_frames)
    assert c.n_frames == n_frames and per.max() <= 3 and c.cap == 4
    if n_frames >= 5:
        assert per[0] == per[n_frames // 2] == per[-1] == 0 and set(per.tolist()) == {0, 1, 2, 3}
        assert np.any(np.diff(c.recs["frame"]) < 0), "frames are not interleaved in memory"


SHEETS = [  # width, height, cell, gap, decimate, tags placed, ids
    (1280, 720, 4, 12, 1, 256, 512), (1280, 720, 4, 12, 1, 257, 512), (1280, 720, 4, 12, 1, 364, 7), (1280, 720, 4, 12, 1, 20, 512),
    (1920, 1080, 6, 18, 2, 364, 7), (1600, 1584, 4, 12, 1, 1024, 512),
]


@pytest.mark.parametrize("sheet", SHEETS, ids=["%dx%d_n%d_mod%d" % (s[0], s[1], s[5], s[6]) for s in SHEETS])
def test_oracle_finds_exactly_the_tags_of_a_sheet(family, sheet):
    w, h, cell, gap, decimate, n, mod = sheet
    assert TS.capacity(family, w, h, cell, gap) >= n
    img = TS.tag_sheet(family, w, h, cell, gap, n=n, ids=lambda k: k % mod)
    ref = O.detect_gray(img, family, decimate)
    assert [r["id"] for r in ref] == sorted(k % mod for k in range(n))
    assert all(r["hamming"] == 0 for r in ref)
