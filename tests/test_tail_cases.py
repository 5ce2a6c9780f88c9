"""The frames of tests/tail_cases.py reach the edges of the per-quad tail they are named after, under the CPU oracle alone
(no GPU needed).  The GPU tests (test_gpu_tail.py) rely on these frames being what they claim.  Nothing here is a
measurement: a case that does not meet its condition is replaced, not skipped."""
import numpy as np
import pytest

import oracle_lib as O
import tail_cases as T


@pytest.fixture(scope="module")
def crops(family):
    """(case, oracle detections, quad report) of every gray cropped case, computed once."""
    return [(c, O.detect_gray(c["gray"], family, c["decimate"], maxhamming=2), T.quad_report(c["gray"], family, c["decimate"]))
            for c in T.cropped_cases(family) if c["frame"].ndim == 2]


def test_crops_cover_the_sides_and_decimations(family):
    have = {(d, s) for d, _, s, _ in T.CROPS}
    assert {(d, s) for d in (1, 2) for s in ("left", "right", "top", "bottom")} <= have
    assert any(d == 3 for d, s in have) and any(d == 4 for d, s in have)
    assert {c for d, c, _, _ in T.CROPS if d == 2} == {8, 12}
    assert all(1 <= k <= 6 for _, _, _, k in T.CROPS)
    for side, tag_id in T.CROP_IDS.items():
        assert T.lost_white_bits(family, tag_id, side) <= 1, side
    cases = T.cropped_cases(family)
    assert len(cases) == 2 * len(T.CROPS) and sum(c["frame"].ndim == 3 for c in cases) == len(T.CROPS)
    for c in cases:
        assert np.array_equal(O.bgr2gray(c["frame"]) if c["frame"].ndim == 3 else c["frame"], c["gray"]), c["name"]


def test_cropped_tags_decode_while_probes_and_sites_leave_the_frame(crops):
    """The oracle returns exactly the placed id with hamming <= 2; one quad has a border sample and a payload site outside
    the frame by SITE_MARGIN or more; and on the right and bottom crops a sample of it has a probe outside
    [0, w - 2] x [0, h - 1] -- under a BGR frame's last pixel.  On the left and top crops no placement of an upright tag puts
    a probe at -1 or below (tail_cases.probe_ends); there a sample has a probe with a coordinate in (-1, 0), which must
    read pixel 0."""
    for c, dets, rep in crops:
        assert [d["id"] for d in dets] == c["ids"] and dets[0]["hamming"] <= 2, (c["name"], dets)
        edge = "leave" if c["side"] in T.HIGH_SIDES else "low"
        hit = [r for r in rep if r[edge].any() and r["border_out"].any() and r["payload_out"].any()]
        assert len(hit) >= 1, (c["name"], [(int(r[edge].sum()), int(r["border_out"].sum()), int(r["payload_out"].sum())) for r in rep])
        if edge == "low":
            assert not any(r["leave"].any() for r in rep), c["name"]


def test_decimate_4_takes_the_step_by_step_loop():
    assert [T.nprobe(f) for f in (1, 2, 3, 4)] == [25, 33, 41, 49]
    assert T.nprobe(3) <= T.DEC_MAX_PROBES < T.nprobe(4)
    assert any(d == 4 for d, _, _, _ in T.CROPS)


def test_sample_totals_are_exact(family):
    assert sorted(T.SAMPLE_CELLS.values()) == [64, 68, 128, 132]
    for c in T.sample_count_cases(family):
        rep = T.quad_report(c["gray"], family, c["decimate"])
        assert c["total"] in [sum(r["ns"]) for r in rep], (c["name"], [r["ns"] for r in rep])
        assert not any(r["leave"].any() for r in rep), c["name"]
        assert [d["id"] for d in O.detect_gray(c["gray"], family, c["decimate"])] == c["ids"], c["name"]


def test_option_frames(family):
    f = T.three_tags(family)
    assert [d["id"] for d in O.detect_gray(f, family, 2, refine_edges=0)] == [20, 21, 22]
    g = T.flipped_cell(family)
    assert O.detect_gray(g, family, 2, maxhamming=0) == []
    two = O.detect_gray(g, family, 2, maxhamming=2)
    assert [(d["id"], d["hamming"]) for d in two] == [(33, 1)]


def test_skip_frame_has_both_kinds_of_rejected_quads(family):
    """Quads the fit passes on (reversed_border = 1, the family's) and the decoder drops: one whose border has the wrong
    polarity (the outlined square: the gray models say brighter outside) and one whose border is right (the hollow square)
    and that no code matches.  Good tags stand beside them."""
    f = T.skip_frame(family)
    dets = O.detect_gray(f, family, 2)
    assert [d["id"] for d in dets] == [0, 4]
    lost = T.undetected(f, family, 2, dets)
    assert all(r["reversed_border"] == 1 for r in lost)
    contrast = [T.border_contrast(f, r["H"], family) for r in lost]
    print("skip frame: border contrast of the undetected quads:", np.round(contrast, 1))
    assert any(c >= 64 for c in contrast), contrast    # "white" (outer) samples brighter: not this family's border
    assert any(c <= -64 for c in contrast), contrast   # right polarity, no detection


def test_batch_outgrows_the_tail_grid(family):
    frames, order = T.batch_frames(family)
    assert len(order) == T.BATCH_N and set(order) == {0, 1}
    nq = [len(T.oracle_quads(f, family, 1)) for f in frames]
    total = sum(nq[k] for k in order)
    print("batch: quads per distinct frame", nq, "total", total)
    assert total > T.TAIL_GRID_MIN and total % T.TAIL_GRID_MIN != 0
    assert max(T.TAIL_GRID_MIN, 64 * T.BATCH_N) == T.TAIL_GRID_MIN
    dets = [O.detect_gray(f, family, 1) for f in frames]
    assert len(dets[0]) == 464 and 0 < len(dets[1]) < len(dets[0])
    lost = T.undetected(frames[1], family, 1, dets[1])
    assert len(lost) >= 100  # inverted tags and hollow squares between the live quads
