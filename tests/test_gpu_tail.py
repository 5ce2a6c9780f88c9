"""The per-quad tail (k_refine, k_homography, k_decode: k_refine.inc, k_decode.inc) on its own edges, with the frames of
tests/tail_cases.py: tags cropped by the frame's edge so that probes, border samples and payload cells fall outside it (gray
and BGR: the last pixel of a BGR frame lies under a probe), quads of exactly one and two passes of 64 edge samples and
four more, the step-by-step probes of decimate 4, refine_edges off, maxhamming 0 and 2, quads the decoder drops for their
border's polarity or for want of a code next to live ones, and a batch with more quads than the tail's grid has
workgroups.  Every frame agrees with the oracle at every stage (check_stages): ids and hamming exactly, corners and centres
to CORNER_TOL, margins as floats.

Not reached by any case: the whole-book search of k_decode (families wider than 48 bits; the library ships none)."""
import numpy as np
import pytest

import oracle_lib as O
import tail_cases as T
from stage_check import CORNER_TOL, check_stages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def detector_for():
    """One detector per option set, shared by the tests of this file."""
    from aprilslam_amd import _lib
    dets = {}

    def get(decimate, maxhamming=1, refine_edges=True):
        key = (decimate, maxhamming, refine_edges)
        if key not in dets:
            dets[key] = _lib.Detector("tagStandard41h12", decimate=float(decimate), maxhamming=maxhamming, refine_edges=refine_edges, id_limit=0)
        return dets[key]
    yield get
    for det in dets.values():
        det.close()


def _no_overflow(det, name):
    cnt = det.debug_counters()
    assert (cnt[11:15] == 0).all(), (name, cnt[11:15])


def _same_as_oracle(dets, ref, name):
    assert [int(d["id"]) for d in dets] == [r["id"] for r in ref], name
    for d, r in zip(dets, ref):
        assert int(d["hamming"]) == r["hamming"], name
        assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL, name
        assert np.abs(d["center"] - r["center"]).max() <= CORNER_TOL, name
        assert np.float32(d["margin"]) == np.float32(r["margin"]), name


def _with_options(det, frame, family, decimate, maxhamming, refine_edges, name):
    """Non-default options: check_stages' oracle runs the defaults, so the detections are compared here."""
    dets, npf = det.detect_host(frame, channels=1 if frame.ndim == 2 else None)
    gray = O.bgr2gray(frame) if frame.ndim == 3 else frame
    ref = O.detect_gray(gray, family, decimate, maxhamming, 1 if refine_edges else 0)
    _same_as_oracle(dets, ref, name)
    _no_overflow(det, name)
    return dets


@pytest.mark.parametrize("decimate", [1, 2, 3, 4])
def test_cropped_tags(detector_for, family, decimate):
    """Every stage with the default options (where the cut-off cells, read as black, cost two bits, oracle and device both
    find nothing), and the detections with maxhamming 2, as the cases were chosen under."""
    cases = [c for c in T.cropped_cases(family) if c["decimate"] == decimate]
    assert cases
    for c in cases:
        check_stages(detector_for(decimate), c["frame"][None], family, decimate=decimate)
        _no_overflow(detector_for(decimate), c["name"])
        dets = _with_options(detector_for(decimate, maxhamming=2), c["frame"], family, decimate, 2, True, c["name"])
        assert [int(d["id"]) for d in dets] == c["ids"], c["name"]


def test_sample_count_edges(detector_for, family):
    for c in T.sample_count_cases(family):
        det = detector_for(c["decimate"])
        dets, npf = check_stages(det, c["frame"][None], family, decimate=c["decimate"])
        assert [int(d["id"]) for d in dets] == c["ids"], c["name"]
        _no_overflow(det, c["name"])


def test_refine_edges_off_and_maxhamming(detector_for, family):
    dets = _with_options(detector_for(2, refine_edges=False), T.three_tags(family), family, 2, 1, False, "refine off")
    assert [int(d["id"]) for d in dets] == [20, 21, 22]
    g = T.flipped_cell(family)
    assert len(_with_options(detector_for(2, maxhamming=0), g, family, 2, 0, True, "maxhamming 0")) == 0
    dets = _with_options(detector_for(2, maxhamming=2), g, family, 2, 2, True, "maxhamming 2")
    assert [(int(d["id"]), int(d["hamming"])) for d in dets] == [(33, 1)]


def test_dropped_quads_beside_live_ones(detector_for, family):
    f = T.skip_frame(family)
    det = detector_for(2)
    dets, npf = check_stages(det, f[None], family, decimate=2)
    assert [int(d["id"]) for d in dets] == [0, 4]
    assert int(det.debug_counters()[5]) >= 6  # the tail saw the dropped quads too
    _no_overflow(det, "skip frame")


def test_batch_beyond_the_grid(family):
    """More quads than workgroups, not a multiple: some workgroups take a second quad, dropped and live ones in turn.  The
    same batch again gives the same bytes, and a one-frame batch after it comes out right: nothing of the large batch's
    per-quad records is left over."""
    import torch
    from aprilslam_amd import _lib
    distinct, order = T.batch_frames(family)
    ref = [O.detect_gray(f, family, 1) for f in distinct]
    nq = [len(T.oracle_quads(f, family, 1)) for f in distinct]
    frames = np.stack([distinct[k] for k in order])
    det = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    try:
        t = torch.from_numpy(frames).to("cuda:0")
        runs = []
        for _ in range(2):
            dets, _, npf = det.detect_device(t.data_ptr(), len(order), 1, T.BATCH_W, T.BATCH_H, max_per_frame=512)
            torch.cuda.synchronize()
            runs.append((dets.copy(), npf.copy()))
            cnt = det.debug_counters()
            assert int(cnt[5]) == sum(nq[k] for k in order) > T.TAIL_GRID_MIN, (int(cnt[5]), nq)
            assert (cnt[11:15] == 0).all(), cnt[11:15]
        dets, npf = runs[0]
        assert npf.tolist() == [len(ref[k]) for k in order]
        starts = np.concatenate([[0], np.cumsum(npf)])
        for b, k in enumerate(order):
            _same_as_oracle(dets[starts[b]:starts[b + 1]], ref[k], "batch frame %d" % b)
        assert runs[1][0].tobytes() == dets.tobytes() and np.array_equal(runs[1][1], npf)
        one, _, npf1 = det.detect_device(t[1:2].data_ptr(), 1, 1, T.BATCH_W, T.BATCH_H, max_per_frame=512)
        torch.cuda.synchronize()
        assert npf1.tolist() == [len(ref[1])]
        _same_as_oracle(one, ref[1], "one frame after the batch")
        del t
    finally:
        det.close()
