"""Stage-by-stage comparison of the HIP detector with the CPU oracle (shared by the GPU parity tests).

Bars: bit-exact for every integer/byte/index product (decimated gray, threshold image, component labels and sizes, tag
ids, hamming, corner order); float products (quad corners, detection corners, margin) are computed with the same IEEE
operations in the same order as the oracle, so they are held to 1e-9 px absolute (observed: identical)."""
import numpy as np

import oracle_lib as O
from aprilslam_amd import synth

CORNER_TOL = 1e-9


def scene_frame(width, height, ntags, seed, noise=0.0):
    rng = np.random.default_rng(seed)
    tags = synth.random_scene(width, height, ntags, rng)
    frame, gt = synth.render_frame(width, height, tags, 18.0, noise_sigma=noise, rng=rng)
    return frame, gt


def check_stages(det, frames, family, decimate=2):
    """frames: (B,H,W,3) or (B,H,W) uint8"""
    dets, npf = det.detect_host(frames, channels=1 if frames.ndim == 3 else None)
    dgray = det.debug_image(0)
    thresh = det.debug_image(1)
    labels = det.debug_image(2)
    sizes = det.debug_image(3)
    quads = det.debug_quads()
    B = frames.shape[0]
    start = 0
    for b in range(B):
        gray = O.bgr2gray(frames[b]) if frames.ndim == 4 else frames[b]
        dec = O.decimate(gray, decimate)
        assert np.array_equal(dgray[b], dec), "decimated gray differs (frame %d)" % b
        th = O.threshold(dec)
        assert np.array_equal(thresh[b], th), "threshold image differs (frame %d)" % b
        lab, sz = O.connected_components(th)
        assert np.array_equal(labels[b], lab), "component labels differ (frame %d)" % b
        roots = lab.ravel() == np.arange(lab.size, dtype=np.uint32)
        assert np.array_equal(sizes[b].ravel()[roots], sz.ravel()[roots]), "component sizes differ (frame %d)" % b
        pts = O.gradient_clusters(th, lab, sz)
        oq = O.fit_quads(dec, pts, family, decimate)
        gq = quads[quads["frame"] == b]
        assert [int(q["cluster"]) for q in gq] == [int(q["cluster"]) for q in oq], "quad clusters differ (frame %d)" % b
        for a, o in zip(gq, oq):
            assert np.abs(a["p"] - o["p"]).max() <= CORNER_TOL, (b, a["p"], o["p"])
        ref = O.detect_gray(gray, family, decimate)
        mine = dets[start:start + npf[b]]
        start += npf[b]
        assert [int(d["id"]) for d in mine] == [r["id"] for r in ref], "ids differ (frame %d)" % b
        for d, r in zip(mine, ref):
            assert int(d["hamming"]) == r["hamming"]
            assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL, (b, d["corners"], r["corners"])
            assert np.abs(d["center"] - r["center"]).max() <= CORNER_TOL
            assert np.float32(d["margin"]) == np.float32(r["margin"])  # same float additions in the same order
    return dets, npf
