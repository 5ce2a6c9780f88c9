"""The point-pass frames of tests/seg_cases.py reach the edges they are named after, under the CPU oracle alone (no GPU
needed).  The GPU tests (test_gpu_seg_points.py) rely on these frames being what they claim."""
import numpy as np
import pytest

import seg_cases as S


@pytest.fixture(scope="module")
def staged():
    """name -> (case, oracle stages), computed once."""
    cases = S.word_seams() + S.tile_seams() + S.sizes() + S.small_components()[0] + [S.table_full()]
    return {c["name"]: (c, S.stages(c["frame"])) for c in cases}


def _of_label(pts, label):
    c = pts["cluster"]
    return pts[((c >> np.uint64(32)) == label) | ((c & np.uint64(0xFFFFFFFF)) == label)]


def test_seam_cases_put_one_cluster_on_their_seam(staged):
    """The square's one cluster (4 x 12 x 2 = 96 points).  Placed at s - 1 and s, pixels on both sides of the seam emit
    its points.  Placed at s + 1 no point can lie across: the square's left (top) points are emitted by column (row) s
    itself, the first of its word (tile), whose neighbour s - 1 is a pixel of the same black ring, staged from across."""
    for fam in (S.word_seams(), S.tile_seams()):
        for c in fam:
            th, lab, sz, pts = staged[c["name"]][1]
            axis, s = c["seam"]
            x, y = c["inside"]
            assert th[y, x] == 255
            mine = _of_label(pts, int(lab[y, x]))
            assert len(np.unique(mine["cluster"])) == 1 and len(mine) == 96 == len(pts), c["name"]
            ex, ey = S.emitters(mine)
            v = ex if axis == "x" else ey
            if c["name"].endswith("+1"):
                assert v.min() == s, c["name"]
                ring = lab == lab[y, x - 7] if axis == "x" else lab == lab[y - 7, x]
                assert th[ring].max() == 0 and ring.sum() >= S.MIN_COMPONENT
                across = ring[:, :s].any() and ring[:, s:].any() if axis == "x" else ring[:s].any() and ring[s:].any()
                assert across, c["name"]
            else:
                assert (v < s).any() and (v >= s).any(), c["name"]


def test_small_blobs_straddle_the_size_floor(staged):
    cases, blobs = S.small_components()
    assert sorted(b["pixels"] for b in blobs) == [24] * 5 + [25] * 5
    for b in blobs:
        th, lab, sz, pts = staged[b["case"]][1]
        x, y = b["at"]
        label = int(lab[y, x])
        comp = lab == label
        assert th[y, x] == 255 and comp.sum() == b["pixels"] == sz.ravel()[label], b["name"]
        assert sorted(zip(*np.nonzero(comp)[::-1])) == sorted(b["cells"])
        n = len(_of_label(pts, label))
        assert (n == 0) if b["pixels"] < S.MIN_COMPONENT else (n >= 24), (b["name"], n)
        cols = np.nonzero(comp.any(axis=0))[0]
        seam = None
        if b["name"].startswith("left pixel"):      # one pixel at x0 - 1 of word 2, the rest in word 2
            seam = 128
            assert comp[:, :128].sum() == 1 and comp[:, 127].sum() == 1 and cols.max() < 192
        elif b["name"].startswith("right pixel"):   # one pixel at x0 + 64 of word 3, the rest in word 3
            seam = 256
            assert comp[:, 256:].sum() == 1 and comp[:, 256].sum() == 1 and cols.min() >= 192
        elif b["name"].startswith("left bar"):      # every pixel is the pixel x0 - 1 of the word on its right
            seam = int(cols[0]) + 1
            assert len(cols) == 1 and seam % S.WORD == 0
        elif b["name"].startswith("right bar"):     # every pixel is the pixel x0 + 64 of the word on its left
            seam = int(cols[0])
            assert len(cols) == 1 and seam % S.WORD == 0
        else:
            assert cols.min() // S.WORD == cols.max() // S.WORD
        # the black ring around it is one large component that the blob touches, on both sides of the seam
        ring = lab == lab[y - 1, x]
        assert th[y - 1, x] == 0 and ring.sum() >= S.MIN_COMPONENT
        if seam is not None:
            assert ring[:, :seam].any() and ring[:, seam:].any()
            if "bar" in b["name"]:
                across = seam - 1 if b["name"].startswith("right") else seam
                assert all(th[yy, across] == 0 and lab[yy, across] == lab[y - 1, x] for _, yy in b["cells"])
                if b["pixels"] >= S.MIN_COMPONENT:
                    # a large bar gets points from the word across the seam: a cluster's worth from the word on its left
                    # (sites (1,0) and (1,1) of every row); the word on its right only adds the (-1,1) point that the
                    # bar's own pixels do not emit first
                    ex, ey = S.emitters(_of_label(pts, label))
                    n = int((ex == across).sum())
                    assert n >= (24 if b["name"].startswith("right") else 1), (b["name"], n)


def test_table_full_frame_fills_the_table_and_stays_common(staged):
    """Counted exactly, the points attributed to the pixel that emits them: one window has more clusters than the
    workgroup's table has slots for (NSLOT - 1), within the common launch's point and run capacities; another overflows the
    points and goes to the dense launch."""
    c, (th, lab, sz, pts) = staged["table full"]
    st = S.window_stats(th, pts)
    assert set(st) == {(0, 0), (0, 63), (0, 126)}
    print("table full: window -> (clusters, points, staged runs):", st)
    assert any(ncl > S.NSLOT - 1 and npt <= S.PCAP and nrun <= S.RUNCAP for ncl, npt, nrun in st.values())
    assert any(npt > S.PCAP for ncl, npt, nrun in st.values())
    assert not S.stays_common(th, pts)


def test_every_other_frame_stays_in_the_common_launch(staged):
    for name, (c, (th, lab, sz, pts)) in staged.items():
        if name != "table full":
            assert S.stays_common(th, pts), name


def test_sizes_cover_the_word_and_tile_edges(staged):
    assert {sw for sw, sh in S.SIZE_PAIRS} == {63, 64, 65, 66, 129, 257}
    assert {sh for sw, sh in S.SIZE_PAIRS} == {62, 63, 64, 65, 127}
    assert len(S.SIZE_PAIRS) == 8
    for c, (sw, sh) in zip(S.sizes(), S.SIZE_PAIRS):
        th, lab, sz, pts = staged[c["name"]][1]
        assert th.shape == (sh, sw)
        assert (th[:, -1] != 127).any() and (th[-1] != 127).any(), c["name"]  # the last column and the last row are coloured
        assert len(S.expected_clusters(pts, sw, sh)) >= 5, c["name"]
        roots = (lab == np.arange(lab.size, dtype=np.uint32).reshape(lab.shape)) & (th != 127)
        assert (sz[roots] < S.MIN_COMPONENT).any() and (sz[roots] >= S.MIN_COMPONENT).any(), c["name"]


def test_expected_clusters_agree_with_the_fit_oracle(staged, family):
    """The helper's per-cluster counts against O.quad_maxima's, the oracle's own path into the quad fit."""
    for name, (c, (th, lab, sz, pts)) in staged.items():
        sh, sw = th.shape
        exp = S.expected_clusters(pts, sw, sh, frame=3)
        st = S.O.quad_maxima(c["frame"], pts, family, 1)
        lo, hi = S.cluster_limits(sw, sh)
        kept = st[(st["count"] >= lo) & (st["count"] <= hi)]
        key = (np.uint64(3) << np.uint64(48)) | ((kept["cluster"] >> np.uint64(32)) << np.uint64(24)) | (kept["cluster"] & np.uint64(0xFFFFFFFF))
        assert np.array_equal(exp[:, 0], key), name
        assert np.array_equal(exp[:, 1], kept["count"].astype(np.uint64)), name
        assert (np.diff(exp[:, 0].astype(np.int64)) > 0).all() and len(set(exp[:, 2].tolist())) == len(exp), name
        assert int(st["count"].sum()) == len(pts)


def test_batch_holds_different_frames_of_one_size():
    frames = [c["frame"] for c in S.batch()]
    assert len(frames) >= 3 and len({f.shape for f in frames}) == 1
    assert len({f.tobytes() for f in frames}) == len(frames)
