"""S0-S3 on their own edges (tests/front_cases.py; tests/test_front_cases.py proves on the CPU that each frame reaches the
edge it is named after): decimation 1, 2, 3, 4 and 8 at every residue of the decimated size, padded input layouts, the
smallest legal frames, the contrast floor and the cut next to its 255 sentinel, the dilation's reach across k_tile_cut's
block seams, the leftover columns and rows, seg_threshold_tile's segments, and the labelling: single contacts on word
seams, row seams and their corner, the last column's diagonal, the border columns, long and late-merging components, the
word-seam pass's same-pair elision, tiles at the capacity of the common launch's tables, and a batch.

For every case all stages agree with the oracle (check_stages: bit-exact up to the corners' CORNER_TOL), the decimated
gray, the threshold image, the labels and the sizes at the roots also equal tests/front_ref.py, the decimate-1 cases
hand the quad fit exactly the clusters the oracle's boundary points give, no overflow counter moves, and the number of tiles
k_seg_tile hands to k_seg_tile_dense is the one counted on the CPU."""
import numpy as np
import pytest

import front_cases as F
import front_ref as R
import oracle_lib as O
import seg_cases as S
from stage_check import check_stages

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def detector_for():
    """One detector per decimation factor, shared by the tests of this file; its workspace follows the frame size."""
    from aprilslam_amd import _lib
    dets = {}

    def get(f):
        if f not in dets:
            dets[f] = _lib.Detector("tagStandard41h12", decimate=float(f), id_limit=0)
        return dets[f]
    yield get
    for det in dets.values():
        det.close()


def _after_batch(det, frames, names, f, dense=None, clusters=True):
    """What holds after every batch, the detector's products still in place: front_ref, the clusters, the counters."""
    dgray, thresh, labels, sizes = (det.debug_image(k) for k in range(4))
    ndense = 0
    for b, frame in enumerate(frames):
        g, th, lab, sz = R.front(frame, f)
        assert np.array_equal(dgray[b], g), (names[b], "decimated gray differs from front_ref")
        assert np.array_equal(thresh[b], th), (names[b], "threshold image differs from front_ref")
        assert np.array_equal(labels[b], lab), (names[b], "labels differ from front_ref")
        roots = lab.ravel() == np.arange(lab.size)
        assert np.array_equal(sizes[b].ravel()[roots], sz.ravel()[roots]), (names[b], "sizes differ from front_ref")
        ndense += F.dense_tiles(th)
    if clusters and f == 1:
        grays = [R.bgr2gray(fr) if fr.ndim == 3 else fr for fr in frames]
        exp = [S.expected_clusters(S.stages(fr)[3], fr.shape[1], fr.shape[0], frame=b) for b, fr in enumerate(grays)]
        exp = np.concatenate(exp)
        got = det.debug_clusters()
        assert got.shape == exp.shape and np.array_equal(got, exp), (names, got.shape, exp.shape)
    cnt = det.debug_counters()
    assert (cnt[11:15] == 0).all(), (names, cnt[11:15])
    assert cnt[17] == ndense, (names, int(cnt[17]), ndense)
    if dense is not None:
        assert ndense == dense, (names, ndense, dense)
    return ndense


def _check(detector_for, family, cases, dense=None):
    """The cases, those of one frame shape and factor as one batch; returns the dense labelling tiles seen.  dense: None, or
    the number of dense labelling tiles a case has unless it says so itself ("dense")."""
    total = 0
    for f, group in F.by_shape(cases):
        names = [c["name"] for c in group]
        frames = np.stack([c["frame"] for c in group])
        det = detector_for(f)
        try:
            check_stages(det, frames, family, decimate=f)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (names, e)) from e
        total += _after_batch(det, frames, names, f, dense=None if dense is None else sum(c.get("dense", dense) for c in group))
    return total


# ------------------------------------------------------------------------------------------------------------------------- A
def test_decimation_at_every_residue(detector_for, family):
    _check(detector_for, family, F.decimation() + F.corner_colours())


def test_smallest_frames(detector_for, family):
    """8 x 8 and 9 x 9: at decimate 3 and 8 the image is smaller than a tile (3 x 3, 1 x 1, 2 x 2), all 127, and the launch
    code skips k_tile_cut; k_seg_tile never reads the cuts then (tw == 0 or th == 0), its masks and the decimation kernel's
    stores are bounded by sw and sh."""
    _check(detector_for, family, F.smallest_frames(), dense=0)


@pytest.mark.parametrize("which", range(3))
def test_padded_layout_through_detect_device(detector_for, family, which):
    """stride = w ch + 5, frame_pitch = stride h + 11, three different frames, the padding alternating 0 / 255: a byte read
    from it would change a gray value or a tile extremum.  The input is read-only."""
    import torch
    name, f, ch, frames = F.padded_layouts()[which]
    buf, stride, pitch = F.pad_batch(frames, ch)
    B, h, w = frames.shape[:3]
    det = detector_for(f)
    t = torch.from_numpy(buf).to("cuda:0")
    dets, _, npf = det.detect_device(t.data_ptr(), B, ch, w, h, stride=stride, frame_pitch=pitch)
    names = ["%s, frame %d" % (name, b) for b in range(B)]
    _after_batch(det, frames, names, f)
    dgray, thresh, labels, sizes = (det.debug_image(k) for k in range(4))
    start = 0
    for b in range(B):
        gray = O.bgr2gray(frames[b]) if ch == 3 else frames[b]
        dec = O.decimate(gray, f)
        th = O.threshold(dec)
        lab, sz = O.connected_components(th)
        assert np.array_equal(dgray[b], dec) and np.array_equal(thresh[b], th) and np.array_equal(labels[b], lab), names[b]
        roots = lab.ravel() == np.arange(lab.size, dtype=np.uint32)
        assert np.array_equal(sizes[b].ravel()[roots], sz.ravel()[roots]), names[b]
        ref = O.detect_gray(gray, family, f)
        mine = dets[start:start + npf[b]]
        start += npf[b]
        assert [int(d["id"]) for d in mine] == [r["id"] for r in ref], names[b]
    assert np.array_equal(t.cpu().numpy(), buf), name
    # the same frames, packed: the same detections
    packed, npf2 = det.detect_host(frames, channels=1 if ch == 1 else None)
    assert np.array_equal(npf, npf2) and packed.tobytes() == dets.tobytes(), name


# ------------------------------------------------------------------------------------------------------------------------- B
def test_contrast_floor_and_cut(detector_for, family):
    cases = F.contrast_floor() + F.leftovers()
    _check(detector_for, family, cases, dense=0)
    det = detector_for(1)
    for c in cases:  # the known answers, straight from the device
        det.detect_host(c["frame"][None], channels=1)
        th = det.debug_image(1)[0]
        assert (th == 127).all() == c["blank"], c["name"]
        for (x, y), v in c["expect"]:
            assert th[y, x] == v, (c["name"], (x, y), int(th[y, x]), v)


def test_dilation_reach(detector_for, family):
    cases = F.dilation_reach()
    _check(detector_for, family, cases, dense=0)
    det = detector_for(1)
    for c in cases:
        det.detect_host(c["frame"][None], channels=1)
        th = det.debug_image(1)[0]
        x0, y0, x1, y1 = c["box"]
        inside = np.zeros(th.shape, bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        assert np.array_equal(th != 127, inside), c["name"]


def test_threshold_segments_noise(detector_for, family):
    n = _check(detector_for, family, [c for c in F.segments() if c["kind"] == "noise"])
    assert n > 0  # per-pixel noise takes the dense labelling launch


def test_threshold_segments_blocks(detector_for, family):
    _check(detector_for, family, [c for c in F.segments() if c["kind"] == "blocks"], dense=0)


# ------------------------------------------------------------------------------------------------------------------------- C
def test_single_contacts(detector_for, family):
    cases = F.single_contacts()
    _check(detector_for, family, cases, dense=0)
    labels = detector_for(1).debug_image(2)  # the last batch: all of them, one frame each
    assert len(labels) == len(cases)
    for c, lab in zip(cases, labels):
        (ax, ay), (bx, by) = c["a"], c["b"]
        assert (lab[ay, ax] == lab[by, bx]) == c["merges"], c["name"]


def test_last_column_and_border_columns(detector_for, family):
    _check(detector_for, family, F.last_column() + F.border_columns(), dense=0)


def test_long_components(detector_for, family):
    cases = F.long_components()
    _check(detector_for, family, cases, dense=0)
    det = detector_for(1)
    labels, sizes = det.debug_image(2), det.debug_image(3)
    for c, lab, sz in zip(cases, labels, sizes):
        th = F.binary(c["frame"])
        for colour, (size, root) in ((255, c["white"]), (0, c["black"])):
            assert sz.ravel()[root] == size and ((lab == root) & (th == colour)).sum() == size, (c["name"], colour)


def test_seam_pairs(detector_for, family):
    _check(detector_for, family, F.seam_pairs(), dense=0)


def test_table_capacity(detector_for, family):
    """511 and 512 runs or links stay in the common launch, 513 go to k_seg_tile_dense: one case a batch, so that counter 17
    is the case's own."""
    for c in F.capacity():
        _check(detector_for, family, [c], dense=c["dense"])


def test_batch_of_different_frames(detector_for, family):
    cases = F.label_batch()
    assert len(F.by_shape(cases)) == 1
    _check(detector_for, family, cases, dense=0)
