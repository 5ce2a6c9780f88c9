"""quad_sigma on the device (k_quad_blur) against the blurred oracle pipeline, composed from the oracle's own stages around
the NumPy statement tests/blur_ref.py: decimate -> quad_blur -> threshold -> components -> clusters -> quad fit.  Everything
the blur can influence is compared as stage_check.check_stages compares it: images, labels and sizes bit for bit, quads by
cluster key with corners within stage_check.CORNER_TOL.  From the edge refinement on, unchanged code reads those quads and
the original frame.

Shapes are the smallest at which the kernel can go wrong: 166 x 125 decimated pixels (no multiple of 4, of the 64 x 16
workgroup tile or of a dword, several workgroups each way), 3 / 5 / 7 / 15 taps (the halo at its smallest and largest),
images a few pixels wider than the kernel, and images narrower than it."""
import functools

import numpy as np
import pytest

import blur_ref
import oracle_lib as O
import stage_check
from aprilslam_amd import _lib
from aprilslam_amd.families import get_family

W, H = 332, 250
# scenes in which the composed oracle pipeline still decodes a tag under the 15-tap blur (chosen with the oracle alone)
SEEDS = (4, 6, 8)
FAMILY = "tagStandard41h12"


@functools.lru_cache(maxsize=None)
def scenes():
    """(frames (3, H, W, 3) BGR, their gray versions, the ground-truth ids per frame); shared, never written to"""
    made = [stage_check.scene_frame(W, H, 3, seed) for seed in SEEDS]
    frames = np.stack([m[0] for m in made])
    gray = np.stack([O.bgr2gray(f) for f in frames])
    frames.setflags(write=False)
    gray.setflags(write=False)
    return frames, gray, [sorted(m[1]) for m in made]


@functools.lru_cache(maxsize=None)
def noisy_frame():
    f = stage_check.scene_frame(W, H, 3, SEEDS[0], noise=6.0)[0][None]
    f.setflags(write=False)
    return f


def small_gray(w, h):
    """a w x h piece of the first scene with a tag edge in it"""
    g = scenes()[1][0]
    ys, xs = np.nonzero(g < 40)
    y0, x0 = max(0, int(ys[0]) - h // 2), max(0, int(xs[0]) - w // 2)
    return np.ascontiguousarray(g[None, y0:y0 + h, x0:x0 + w])


def oracle_stages(gray, decimate, s):
    """the blurred oracle pipeline of one gray frame"""
    fam = get_family(FAMILY)
    dec = O.decimate(gray, decimate)
    q = blur_ref.quad_blur(dec, s)
    th = O.threshold(q)
    lab, sz = O.connected_components(th)
    pts = O.gradient_clusters(th, lab, sz)
    return dict(dec=dec, q=q, th=th, lab=lab, sz=sz, quads=O.fit_quads(q, pts, fam, decimate))


def check_blur_stages(det, frames, decimate, s):
    """frames (B, H, W, 3) or (B, H, W): every stage the blur reaches, device against oracle; returns (dets, npf)"""
    det.set_quad_sigma(s)
    try:
        dets, npf = det.detect_host(frames, channels=1 if frames.ndim == 3 else None)
        image, plain = det.debug_image(0), det.debug_image(9)
        thresh, labels, sizes, quads = det.debug_image(1), det.debug_image(2), det.debug_image(3), det.debug_quads()
    finally:
        det.set_quad_sigma(0)
    for b in range(frames.shape[0]):
        o = oracle_stages(O.bgr2gray(frames[b]) if frames.ndim == 4 else frames[b], decimate, s)
        assert np.array_equal(plain[b], o["dec"]), "decimated gray differs (frame %d)" % b
        bad = np.argwhere(image[b] != o["q"])
        assert len(bad) == 0, "blurred image differs at %d pixels, first (y, x) = %s (frame %d)" % (len(bad), bad[0], b)
        assert np.array_equal(thresh[b], o["th"]), "threshold image differs (frame %d)" % b
        assert np.array_equal(labels[b], o["lab"]), "component labels differ (frame %d)" % b
        roots = o["lab"].ravel() == np.arange(o["lab"].size, dtype=np.uint32)
        assert np.array_equal(sizes[b].ravel()[roots], o["sz"].ravel()[roots]), "component sizes differ (frame %d)" % b
        gq = quads[quads["frame"] == b]
        assert [int(q["cluster"]) for q in gq] == [int(q["cluster"]) for q in o["quads"]], "quad clusters differ (frame %d)" % b
        for a, q in zip(gq, o["quads"]):
            assert np.abs(a["p"] - q["p"]).max() <= stage_check.CORNER_TOL, (b, a["p"], q["p"])
    return dets, npf


@pytest.fixture(scope="module")
def detectors():
    """one detector per decimation factor, made on first use"""
    made = {}

    def get(decimate):
        if decimate not in made:
            made[decimate] = _lib.Detector(FAMILY, decimate=float(decimate), id_limit=0)
        return made[decimate]
    yield get
    for d in made.values():
        d.close()


def test_seeds_give_quads_on_every_frame():
    """no GPU: the scenes are worth comparing -- the composed oracle finds candidate quads on every frame under every sigma"""
    _, gray, ids = scenes()
    assert all(i == [0, 1, 2] for i in ids)
    for s in (0.8, -0.8, 1.9, 3.9):
        for b in range(len(SEEDS)):
            assert len(oracle_stages(gray[b], 2, s)["quads"]) > 0, (s, b)


@pytest.mark.gpu
@pytest.mark.parametrize("s", [0.8, -0.8, 1.9, 3.9])
def test_bgr_batch_matches_the_blurred_oracle(detectors, s):
    """3, 7 and 15 taps, blur and sharpening; end to end every frame still yields a tag, and only tags of its scene"""
    frames, _, ids = scenes()
    dets, npf = check_blur_stages(detectors(2), frames, 2, s)
    assert (np.asarray(npf) >= 1).all(), npf
    start = 0
    for b, n in enumerate(npf):
        assert set(int(i) for i in dets["id"][start:start + n]) <= set(ids[b]), (b, dets["id"][start:start + n])
        start += n


@pytest.mark.gpu
@pytest.mark.parametrize("decimate", [1, 3])
def test_gray_batch_other_decimations(detectors, decimate):
    """332 x 250 (rows of whole dwords: the aligned loads and stores) and 111 x 84 (odd), 5 taps"""
    check_blur_stages(detectors(decimate), scenes()[1], decimate, 1.25)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,s", [(24, 20, 1.9), (8, 8, 0.8), (8, 8, 1.9)])
def test_images_about_as_wide_as_the_kernel(detectors, w, h, s):
    """12 x 10 under 7 taps: 5 x 3 filtered pixels; 4 x 4 under 3 taps: one; 4 x 4 under 7 taps: all copied"""
    frames = small_gray(w, h)
    assert frames.shape == (1, h, w) and frames.min() < 40 and frames.max() > 100
    check_blur_stages(detectors(2), frames, 2, s)
    dec = O.decimate(frames[0], 2)
    nfilt = max(0, dec.shape[0] - 2 * (len(blur_ref.blur_taps(s)) // 2) - 1) * max(0, dec.shape[1] - 2 * (len(blur_ref.blur_taps(s)) // 2) - 1)
    assert nfilt == {(24, 1.9): 15, (8, 0.8): 1, (8, 1.9): 0}[(w, s)]
    if nfilt == 0:
        assert np.array_equal(blur_ref.quad_blur(dec, s), dec)


@pytest.mark.gpu
def test_noisy_frame(detectors):
    """sensor noise: the dense-tile paths of the segmentation see the blurred noise"""
    check_blur_stages(detectors(2), noisy_frame(), 2, 0.8)


def _everything(det, frames):
    """results and debug items of one batch as bytes.  Item 3 holds a component's size at its label (asl_debug_fetch:
    "sizes by label"); the other entries of that buffer are never written, so they are whatever the memory held and
    only the entries at the labels are taken."""
    dets, npf = det.detect_host(frames)
    gray, thresh, labels, sizes = (det.debug_image(k) for k in (0, 1, 2, 3))
    at_label = labels.reshape(len(labels), -1) == np.arange(labels[0].size, dtype=np.uint32)
    return [dets.tobytes(), np.asarray(npf).tobytes(), gray.tobytes(), thresh.tobytes(), labels.tobytes(),
            sizes.reshape(len(sizes), -1)[at_label].tobytes(), det.debug_quads().tobytes()]


@pytest.mark.gpu
def test_switching_off_restores_the_plain_detector(detectors):
    frames = scenes()[0]
    fresh = _lib.Detector(FAMILY, id_limit=0)
    try:
        want = _everything(fresh, frames)
        assert np.array_equal(fresh.debug_image(9), fresh.debug_image(0))  # blur off: item 9 is item 0
    finally:
        fresh.close()
    det = detectors(2)
    det.set_quad_sigma(0.8)
    try:
        blurred = _everything(det, frames)
        assert blurred[2] != want[2]
        det.set_quad_sigma(0)
        assert _everything(det, frames) == want
        det.set_quad_sigma(0.4)  # ksz = 1: accepted, and off
        assert _everything(det, frames) == want
        for bad in (4.0, -4.0, float("nan"), float("inf")):
            with pytest.raises(_lib.AslError):
                det.set_quad_sigma(bad)
        assert _everything(det, frames) == want  # a refused value changes nothing
    finally:
        det.set_quad_sigma(0)


@pytest.mark.gpu
def test_setter_refused_while_a_batch_is_pending(detectors):
    import torch
    frames = scenes()[0]
    det = detectors(2)
    t = torch.from_numpy(np.array(frames)).to("cuda:0")
    det.submit_device(t.data_ptr(), frames.shape[0], 3, W, H)
    try:
        with pytest.raises(_lib.AslError):
            det.set_quad_sigma(0.8)
    finally:
        dets, _, npf = det.collect()
    assert (np.asarray(npf) >= 1).all()
    det.set_quad_sigma(0.8)  # collected: accepted again
    det.set_quad_sigma(0)


@pytest.mark.gpu
def test_same_batch_twice_gives_the_same_bytes(detectors):
    frames = scenes()[0]
    det = detectors(2)
    det.set_quad_sigma(-1.25)
    try:
        first = _everything(det, frames)
        assert _everything(det, frames) == first
    finally:
        det.set_quad_sigma(0)


@pytest.mark.gpu
def test_shim_and_tag_detector_take_the_knob():
    """apriltag(family, blur=s) and TagDetector(..., quad_sigma=s): the drop-in call surface reaches the setter"""
    from aprilslam_amd.apriltag import apriltag
    from aprilslam_amd.tag_detector import TagDetector
    _, gray, ids = scenes()
    plain = apriltag(FAMILY, id_limit=0)
    soft = apriltag(FAMILY, blur=0.8, id_limit=0)
    got = soft.detect(gray[0])
    assert sorted(d["id"] for d in got) == ids[0] == sorted(d["id"] for d in plain.detect(gray[0]))
    assert np.array_equal(soft._det.debug_image(0)[0], blur_ref.quad_blur(O.decimate(gray[0], 2), 0.8))
    assert np.array_equal(plain._det.debug_image(0)[0], O.decimate(gray[0], 2))
    with pytest.raises(RuntimeError):
        apriltag(FAMILY, blur=4.0)
    td = TagDetector({"camera_matrix": np.eye(3), "dist_coeffs": np.zeros((4, 1))}, id_limit=0, quad_sigma=-0.8)
    td.detect(gray[0])
    assert np.array_equal(td.detector._det.debug_image(0)[0], blur_ref.quad_blur(O.decimate(gray[0], 2), -0.8))
