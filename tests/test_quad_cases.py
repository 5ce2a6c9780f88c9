"""The quad-fit edge cases of tests/quad_cases.py hit their targets under the CPU oracle (no GPU needed): exact raw point
counts on both sides of every size-class cap, the 24-point floor and the upper limit, and the maxima conditions of the
10-maxima cap.  The GPU tests (test_gpu_quad_classes.py) rely on these frames being what they claim."""
import numpy as np
import pytest

import quad_cases as Q


@pytest.mark.parametrize("scale", [1, 2])
def test_edge_frames_hit_their_counts_and_maxima(family, scale):
    frames, cases = Q.edge_frames(scale)
    recs = Q.case_records(frames, cases, family, scale)
    counts = set()
    for c, r in zip(cases, recs):
        assert int(r["count"]) == c["count"], (c["name"], int(r["count"]))
        counts.add(c["count"])
        if c["count"] < 24:
            assert r["unique"] == -1 and not r["fitted"], c["name"]   # dropped before the fit
            continue
        assert r["unique"] == c["count"], c["name"]                   # rectangles have no duplicate points
        m = c["maxima"]
        if m in (4, 10):
            assert r["nmaxima"] == m and r["nkept"] == m and not r["tie"], (c["name"], int(r["nmaxima"]))
        elif m == ">10":
            assert r["nmaxima"] > 10 and r["nkept"] == 10 and not r["tie"], (c["name"], int(r["nmaxima"]))
        elif m == "tie":
            assert r["nmaxima"] > 10 and r["nkept"] < 10 and r["tie"], (c["name"], int(r["nmaxima"]))
    for cap in Q.CLASS_CAPS:
        assert {cap, cap + 1} <= counts
    assert {23, 24} <= counts
    assert sum(Q.size_class(n) == 4 for n in counts) >= 4
    # every size class fits at least one quad among the cases, and tags are found in both frames
    fitted = {Q.size_class(c["count"]) for c, r in zip(cases, recs) if r["fitted"]}
    assert fitted == {0, 1, 2, 3, 4}
    for b in range(len(frames)):
        assert len(Q.O.detect_gray(frames[b], family, scale)) >= 3


@pytest.mark.parametrize("scale", [1, 2])
def test_limit_frames_straddle_the_upper_limit(family, scale):
    frames, cases = Q.limit_frames(scale)
    L = Q.upper_limit(Q.LIMIT_WH, Q.LIMIT_WH)
    recs = Q.case_records(frames, cases, family, scale)
    assert [int(r["count"]) for r in recs] == [L, L + 1] == [c["count"] for c in cases]
    assert recs[0]["unique"] == L and recs[0]["nmaxima"] > 10     # kept: the fit runs (and rejects it)
    assert recs[1]["unique"] == -1                                # dropped by the size filter


def test_batch_textures_fill_their_class(family):
    for cls, frame in Q.batch_textures().items():
        dec, lab, pts, st = Q.oracle_stages(frame, family, 1)
        kept = st[(st["count"] >= 24) & (st["count"] <= Q.upper_limit(dec.shape[1], dec.shape[0]))]
        classes = np.array([Q.size_class(int(n)) for n in kept["count"]])
        if cls == "tags":
            assert len(Q.O.detect_gray(frame, family, 1)) == 12
            continue
        assert len(classes) > 100 and (classes == cls).all(), cls
        assert kept["fitted"].mean() > 0.95, cls                  # the fits run to the end: corners are compared
