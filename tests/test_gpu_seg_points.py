"""The point pass (k_seg_points, k_seg.inc) on its own edges, at decimate 1 on gray frames (tests/seg_cases.py): squares on
word seams and point-tile seams, frame sizes around one and two words and tiles, components on both sides of the 25-pixel
floor beside a seam, a workgroup whose cluster table fills up (its points probe the global table one by one) next to
workgroups that hand their tiles to the dense launch, and one batch of different frames.  For every frame all stages agree
with the oracle (check_stages) and the clusters the quad fit receives -- keys, order, counts and the hash of the sorted
point records -- are exactly those the oracle's boundary points give (seg_cases.expected_clusters).

Not reached by any case: the table-full fallback of the DENSE instantiation (more than 255 clusters within half a tile
that already overflowed the common launch); it shares segp_emit and the run lookup with the common launch's, which the
table-full frame exercises."""
import numpy as np
import pytest

import seg_cases as S
from stage_check import check_stages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def detector_for():
    """One detector per frame size, shared by the tests of this file."""
    from aprilslam_amd import _lib
    dets = {}

    def get(shape):
        if shape not in dets:
            dets[shape] = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
        return dets[shape]
    yield get
    for det in dets.values():
        det.close()


def _check(detector_for, family, cases, dense):
    """Every case alone, as a batch of one frame."""
    for c in cases:
        f = c["frame"]
        det = detector_for(f.shape)
        check_stages(det, f[None], family, decimate=1)
        th, lab, sz, pts = S.stages(f)
        exp = S.expected_clusters(pts, f.shape[1], f.shape[0])
        got = det.debug_clusters()
        assert got.shape == exp.shape and np.array_equal(got, exp), (c["name"], got.shape, exp.shape)
        cnt = det.debug_counters()
        assert (cnt[11:15] == 0).all(), (c["name"], cnt[11:15])
        assert (cnt[16] > 0) if dense else (cnt[16] == 0), (c["name"], int(cnt[16]))


def test_word_seams(detector_for, family):
    _check(detector_for, family, S.word_seams(), dense=False)


def test_point_tile_seams(detector_for, family):
    _check(detector_for, family, S.tile_seams(), dense=False)


def test_frame_sizes(detector_for, family):
    _check(detector_for, family, S.sizes(), dense=False)


def test_small_components_beside_a_seam(detector_for, family):
    _check(detector_for, family, S.small_components()[0], dense=False)


def test_cluster_table_full_and_handover(detector_for, family):
    _check(detector_for, family, [S.table_full()], dense=True)


def test_batch_of_different_frames(detector_for, family):
    """Frame-major grid and per-frame cursor: every frame's clusters carry its own frame number and its own points."""
    frames = np.stack([c["frame"] for c in S.batch()])
    det = detector_for(frames.shape[1:])
    check_stages(det, frames, family, decimate=1)
    exp = np.concatenate([S.expected_clusters(S.stages(f)[3], f.shape[1], f.shape[0], frame=b) for b, f in enumerate(frames)])
    got = det.debug_clusters()
    assert len(exp) >= len(frames) and got.shape == exp.shape and np.array_equal(got, exp)
    cnt = det.debug_counters()
    assert (cnt[11:15] == 0).all() and cnt[16] == 0
