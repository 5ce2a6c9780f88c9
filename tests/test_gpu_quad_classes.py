"""The quad fit (k_quad.inc) in every size class against the oracle: clusters on both sides of each class cap, the
24-point floor, the upper limit and the 10-maxima cap (tests/quad_cases.py), and every class at batch scale, where each
class holds more than three times as many clusters as its grid has workgroups, so the grid-stride loop and the clamped
prefetch of the class list run to their ragged tails."""
import numpy as np
import pytest

import quad_cases as Q
from stage_check import CORNER_TOL, check_stages

pytestmark = pytest.mark.gpu

# distinct batch frames (quad_cases.batch_textures) and how often each appears: every class gets more than 3 G clusters
BATCH_MULT = {0: 19, 1: 38, 2: 14, 3: 20, 4: 49, "tags": 3}


def _gpu_clusters(det):
    """frame, frame-local cluster id ((hi << 32) + lo, the oracle's) and raw point count of every cluster the fit received."""
    cl = det.debug_clusters()
    key = cl[:, 0]
    frame = (key >> np.uint64(48)).astype(np.int64)
    cid = (((key >> np.uint64(24)) & np.uint64(0xFFFFFF)) << np.uint64(32)) + (key & np.uint64(0xFFFFFF))
    return frame, cid, cl[:, 1].astype(np.int64)


def _fit_grids(det, B):
    """Workgroups of each class's grid-stride loop, as launch_fit_class (aprilslam.hip) sizes them."""
    mc = int(det.debug_counters()[8])
    small = min(mc, max(16384, 32 * B))
    return [small, small, min(mc, 2048), min(mc, 2048), min(mc, 2048)]


@pytest.mark.parametrize("scale", [1, 2])
def test_edge_frames_stage_parity(family, scale):
    """Decimate 1, and decimate 2 on the same shapes scaled x 2: every stage bit-exact, and the GPU's own clusters carry
    each case's exact raw point count; those outside [24, L] are absent on both sides."""
    from aprilslam_amd import _lib
    det = _lib.Detector("tagStandard41h12", decimate=float(scale), id_limit=0)
    try:
        for build in (Q.edge_frames, Q.limit_frames):
            frames, cases = build(scale)
            dets, npf = check_stages(det, frames, family, decimate=scale)
            sh, sw = frames.shape[1] // scale, frames.shape[2] // scale
            L = Q.upper_limit(sw, sh)
            fr, cid, cnt = _gpu_clusters(det)
            quads = det.debug_quads()
            for c, r in zip(cases, Q.case_records(frames, cases, family, scale)):
                mine = (fr == c["frame"]) & (cid == r["cluster"])
                if 24 <= c["count"] <= L:
                    assert mine.sum() == 1 and cnt[mine][0] == c["count"], (c["name"], cnt[mine])
                else:
                    assert mine.sum() == 0, c["name"]
                    assert not ((quads["frame"] == c["frame"]) & (quads["cluster"] == r["cluster"])).any(), c["name"]
            if build is Q.edge_frames:
                assert (npf >= 3).all()
    finally:
        det.close()


def _oracle_frame(frame, family):
    dec, lab, pts, st = Q.oracle_stages(frame, family, 1)
    oq = Q.O.fit_quads(dec, pts, family, 1, cap=8192)
    L = Q.upper_limit(dec.shape[1], dec.shape[0])
    kept = st["count"][(st["count"] >= 24) & (st["count"] <= L)]
    return dict(cluster=np.array([int(q["cluster"]) for q in oq], dtype=np.uint64),
                p=np.array([q["p"] for q in oq]).reshape(-1, 4, 2),
                classes=np.bincount([Q.size_class(int(n)) for n in kept], minlength=5),
                dets=Q.O.detect_gray(frame, family, 1))


def _compare_batch(det, frames, keys, ref, dets, npf):
    """Every frame's quads (cluster ids and corners) and detections against the oracle of its distinct frame."""
    ncl = int(det.debug_counters()[3])
    quads = det.debug_quads(cap=ncl + 1)
    bounds = np.searchsorted(quads["frame"], np.arange(len(frames) + 1))
    starts = np.concatenate([[0], np.cumsum(npf)])
    for b, k in enumerate(keys):
        gq, o = quads[bounds[b]:bounds[b + 1]], ref[k]
        assert np.array_equal(gq["cluster"], o["cluster"]), "quad clusters differ (frame %d, %s)" % (b, k)
        if len(gq):
            assert np.abs(gq["p"] - o["p"]).max() <= CORNER_TOL, (b, k)
        mine = dets[starts[b]:starts[b + 1]]
        assert [int(d["id"]) for d in mine] == [r["id"] for r in o["dets"]], (b, k)
        for d, r in zip(mine, o["dets"]):
            assert int(d["hamming"]) == r["hamming"]
            assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL, (b, k)


@pytest.fixture(scope="module")
def batch_run(family):
    """One device batch of ~140 decimate-1 frames in a seeded order, on a detector the leftover-state test reuses."""
    import torch
    from aprilslam_amd import _lib
    tex = Q.batch_textures()
    keys = [k for k, n in BATCH_MULT.items() for _ in range(n)]
    keys = [keys[i] for i in np.random.default_rng(11).permutation(len(keys))]
    frames = np.stack([tex[k] for k in keys])
    ref = {k: _oracle_frame(f, family) for k, f in tex.items()}
    det = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    t = torch.from_numpy(frames).to("cuda:0")
    B = len(keys)
    dets, _, npf = det.detect_device(t.data_ptr(), B, 1, Q.W, Q.H)
    torch.cuda.synchronize()
    yield det, frames, keys, ref, dets.copy(), npf
    del t
    det.close()


def test_batch_scale_every_class_iterates(batch_run):
    """Each class holds more than 3 G clusters, G its grid (not a multiple of G): every workgroup runs at least three
    iterations of the grid-stride loop and the three-deep prefetch meets the clamped end of the class list.  All quads of
    every frame and all detections are compared with the oracle."""
    det, frames, keys, ref, dets, npf = batch_run
    B = len(keys)
    c = det.debug_counters()
    assert c[11] == 0 and c[12] == 0 and c[13] == 0 and c[14] == 0
    fr, cid, cnt = _gpu_clusters(det)
    per_class = np.bincount([Q.size_class(int(n)) for n in cnt], minlength=5)
    expect = sum(ref[k]["classes"] for k in keys)
    assert np.array_equal(per_class, expect), (per_class, expect)
    grids = _fit_grids(det, B)
    iters = []
    for cls in range(5):
        G = grids[cls]
        assert per_class[cls] > 3 * G and per_class[cls] % G != 0, (cls, int(per_class[cls]), G)
        iters.append((int(per_class[cls]), G, -(-int(per_class[cls]) // G)))
    print("batch %d frames; per class (clusters, grid, iterations of the busiest workgroup): %s" % (B, iters))
    _compare_batch(det, frames, keys, ref, dets, npf)


def test_smaller_batch_after_large_one_has_no_leftover_quads(batch_run, family):
    """The quad records persist between batches: after the large batch, a smaller one on the same detector must come out
    exactly as the oracle says, so no cluster of it was skipped and left showing an old record."""
    det = batch_run[0]
    frames, _ = Q.edge_frames(1)
    check_stages(det, frames, family, decimate=1)
    tex = Q.batch_textures()
    small = np.stack([tex[2], tex[0], tex["tags"]])
    dets, npf = det.detect_host(small, channels=1)
    keys = [2, 0, "tags"]
    ref = {k: _oracle_frame(tex[k], family) for k in set(keys)}
    _compare_batch(det, small, keys, ref, dets, npf)
