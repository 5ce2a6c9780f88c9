"""Deterministic gray frames on the edges of the point pass (k_seg_points, k_seg.inc), for decimate 1: every pixel is
the test's own.  The pass works on words of 64 pixels (one wavefront each, four to a workgroup: 256 pixels) and on point
tiles of 63 emitting rows that stage a 64th; a workgroup's window is therefore 256 x 63 pixels at (256 i, 63 j).

expected_clusters() restates, from the oracle's boundary points, what Detector.debug_clusters() returns;
tests/test_seg_cases.py checks under the oracle alone that every case reaches the edge it is named after.
"""
import numpy as np

import oracle_lib as O

DARK, LIGHT, GROUND = 40, 215, 127
WORD, TILE_ROWS, GROUP = 64, 63, 256      # pixels of a word, emitting rows of a point tile, pixels of a workgroup's words
NSLOT, PCAP, RUNCAP = 256, 4096, 2048     # SEGP_NSLOT, SEGP_PCAP, SEGP_RUNCAP of k_seg.inc
MIN_COMPONENT = 25

_GCODE = {0: 0, 255: 1, -255: 2}


def stages(gray):
    """The oracle's threshold image, labels, sizes and boundary points of one gray frame at decimate 1."""
    dec = O.decimate(gray, 1)
    th = O.threshold(dec)
    lab, sz = O.connected_components(th)
    return th, lab, sz, O.gradient_clusters(th, lab, sz)


def cluster_limits(sw, sh):
    return 24, 3 * (2 * sw + 2 * sh)  # k_cluster_filter's rule


def expected_clusters(pts, sw, sh, frame=0):
    """(n, 3) uint64 as Detector.debug_clusters() returns them for this frame: key = frame << 48 | hi << 24 | lo, point
    count, FNV-1a over the sorted packed records x | y << 16 | gx code << 32 | gy code << 34 (codes 0: 0, 1: +255, 2: -255);
    the clusters k_cluster_filter keeps, ordered by key."""
    lo_n, hi_n = cluster_limits(sw, sh)
    out = []
    ids, starts = np.unique(pts["cluster"], return_index=True)  # the oracle returns the points sorted by cluster
    bounds = list(starts) + [len(pts)]
    for k, cid in enumerate(ids):
        p = pts[bounds[k]:bounds[k + 1]]
        if not lo_n <= len(p) <= hi_n:
            continue
        hi, lo = int(cid) >> 32, int(cid) & 0xFFFFFFFF
        recs = sorted(int(q["x"]) | int(q["y"]) << 16 | _GCODE[int(q["gx"])] << 32 | _GCODE[int(q["gy"])] << 34 for q in p)
        h = 0xcbf29ce484222325
        for r in recs:
            h = ((h ^ r) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        out.append((frame << 48 | hi << 24 | lo, len(p), h))
    out.sort()
    return np.array(out, dtype=np.uint64).reshape(-1, 3)


def emitters(pts):
    """(x, y) of the pixel that emits each point: a point is pixel (x, y) + (dx, dy) / 2 at doubled coordinates, its sites
    are (1,0), (0,1), (-1,1), (1,1); for the diagonals dx is the sign of gx * gy."""
    X, Y = pts["x"].astype(np.int64), pts["y"].astype(np.int64)
    dy = Y & 1
    dx = np.where(dy == 0, 1, np.where(X & 1 == 0, 0, np.sign(pts["gx"].astype(np.int64) * pts["gy"].astype(np.int64))))
    return (X - dx) // 2, (Y - dy) // 2


def staged_runs(th, x0, y0):
    """Run entries the workgroup of window (x0, y0) stages: over its 64 rows and four words, a word's own runs plus its
    coloured neighbour pixels x - 1 and x + 64; a word without a coloured pixel in those rows stages nothing.  Pixel
    sw - 1 never joins its left neighbour."""
    sh, sw = th.shape
    rows = th[y0:min(y0 + TILE_ROWS + 1, sh)]
    total = 0
    for wx0 in range(x0, min(x0 + GROUP, sw), WORD):
        w = rows[:, wx0:min(wx0 + WORD, sw)]
        col = w != 127
        if not col.any():
            continue
        start = col.copy()
        start[:, 1:] &= w[:, 1:] != w[:, :-1]
        if wx0 + WORD >= sw:
            start[:, -1] = col[:, -1]
        total += int(start.sum())
        if wx0 > 0:
            total += int((rows[:, wx0 - 1] != 127).sum())
        if wx0 + WORD < sw:
            total += int((rows[:, wx0 + WORD] != 127).sum())
    return total


def window_stats(th, pts):
    """{(x0, y0): (clusters, points, staged runs)} of every workgroup window of the common launch, the points attributed
    to the pixel that emits them."""
    sh, sw = th.shape
    ex, ey = emitters(pts)
    out = {}
    for y0 in range(0, max(sh - 1, 1), TILE_ROWS):
        for x0 in range(0, sw, GROUP):
            m = (ex >= x0) & (ex < x0 + GROUP) & (ey >= y0) & (ey < y0 + TILE_ROWS)
            out[(x0, y0)] = (len(np.unique(pts["cluster"][m])), int(m.sum()), staged_runs(th, x0, y0))
    return out


def stays_common(th, pts):
    """No window of the frame exceeds the common launch's run or point capacity: no tile goes to the dense launch."""
    return all(p <= PCAP and r <= RUNCAP for _, p, r in window_stats(th, pts).values())


def _square(frame, x, y, n=12):
    frame[y:y + n, x:x + n] = LIGHT


def word_seams():
    """A 12 x 12 white square on a dark ground, its left edge at s - 1, s, s + 1 for the word seams s = 64, 128 (inside a
    workgroup) and 256 (between workgroups); frames 330 x 40."""
    cases = []
    for s in (64, 128, 256):
        for d in (-1, 0, 1):
            f = np.full((40, 330), DARK, np.uint8)
            _square(f, s + d, 14)
            cases.append(dict(name="word seam %d%+d" % (s, d), frame=f, seam=("x", s), inside=(s + d + 5, 19)))
    return cases


def tile_seams():
    """The same square with its top edge at t - 1, t, t + 1 for t = 63 and 126: row 63 is the "row below" of point tile 0
    and row 0 of tile 1; frames 80 x 140."""
    cases = []
    for t in (63, 126):
        for d in (-1, 0, 1):
            f = np.full((140, 80), DARK, np.uint8)
            _square(f, 30, t + d)
            cases.append(dict(name="tile seam %d%+d" % (t, d), frame=f, seam=("y", t), inside=(35, t + d + 5)))
    return cases


SIZE_PAIRS = ((63, 62), (64, 63), (65, 64), (66, 65), (129, 127), (257, 63), (64, 65), (129, 62))  # (sw, sh)


def sizes():
    """Frame sizes around one and two words and one and two point tiles, textured up to the last column and row with a
    seeded pattern of 4 x 4 pixel blocks (one in six white), so pixel sw - 1 and row sh - 1 are coloured."""
    cases = []
    for k, (sw, sh) in enumerate(SIZE_PAIRS):
        rng = np.random.default_rng(100 + k)
        blocks = rng.random(((sh + 3) // 4, (sw + 3) // 4)) < 1 / 6
        f = np.where(blocks.repeat(4, axis=0).repeat(4, axis=1)[:sh, :sw], LIGHT, DARK).astype(np.uint8)
        cases.append(dict(name="size %dx%d" % (sw, sh), frame=f))
    return cases


def _blob(frame, cells):
    for x, y in cells:
        frame[y, x] = LIGHT


def small_components():
    """White blobs of 24 pixels (deleted as too small) and 25 pixels (kept) on a dark ground, whose surrounding black ring
    is one large component on both sides of every seam; two 330 x 40 frames.
    Frame "small components": "inside": the blob lies within a word.  "left pixel": its body lies in the word right of
    seam 128 and a single pixel of it at column 127, the pixel x0 - 1 of that word.  "right pixel": its body lies left of
    seam 256 and a single pixel at column 256, the pixel x0 + 64 of the word on the left.
    Frame "small bars": one-pixel columns 24 and 25 rows high in the first or last column of a word, so that the word
    across the seam sees a small component in its neighbour pixel of every row: were the deletion of the pixel x0 + 64
    forgotten, the word on the left would emit a cluster's worth of points (one pixel's few fall below the cluster floor).
    "right bar": column 256 (24) and 64 (25), the pixel x0 + 64 of the word on the left; "left bar": column 127 (24) and
    191 (25), the pixel x0 - 1 of the word on the right.
    Returns the two cases and the blobs: {case, name, pixels, cells, (x, y) of one of its pixels}."""
    f = np.full((40, 330), DARK, np.uint8)
    g = np.full((40, 330), DARK, np.uint8)
    blobs = []
    for npx, y in ((24, 6), (25, 24)):
        def body(x):
            cells = [(x + i, y + j) for j in range(4) for i in range(6)]
            return cells[:-1] if npx == 24 else cells  # 23 or 24 pixels, one more follows
        for name, cells in (("inside", body(20) + [(26, y)]),
                            ("left pixel", body(128) + [(127, y + 1)]),
                            ("right pixel", body(250) + [(256, y + 1)])):
            assert len(set(cells)) == npx
            _blob(f, cells)
            blobs.append(dict(case="small components", name="%s %d" % (name, npx), pixels=npx, cells=cells, at=cells[0]))
    for name, x, npx in (("right bar", 256, 24), ("right bar", 64, 25), ("left bar", 127, 24), ("left bar", 191, 25)):
        cells = [(x, 8 + j) for j in range(npx)]
        _blob(g, cells)
        blobs.append(dict(case="small bars", name="%s %d" % (name, npx), pixels=npx, cells=cells, at=cells[0]))
    return [dict(name="small components", frame=f), dict(name="small bars", frame=g)], blobs


def table_full():
    """256 x 189, ground 127: two bands of one-pixel columns 25 rows high (white at odd x, black at even x, x = 1 .. 254)
    at rows 40 .. 64 and 124 .. 148, and six 6 x 6 white squares in 2-pixel black frames between them.  The window of rows
    63 .. 125 sees two rows of each band: more clusters than the workgroup's table has slots, yet few enough points and runs
    to stay in the common launch; the windows above and below hold a band's bulk and go to the dense launch."""
    f = np.full((189, 256), GROUND, np.uint8)
    for y0 in (40, 124):
        f[y0:y0 + 25, 1:255:2] = 255
        f[y0:y0 + 25, 2:255:2] = 0
    for k in range(6):
        x = 20 + 38 * k
        f[88:98, x:x + 10] = 0
        f[90:96, x + 2:x + 8] = 255
    return dict(name="table full", frame=f)


def batch():
    """Five different 330 x 40 frames for one device batch."""
    w = word_seams()
    return [w[1], w[3], w[8]] + small_components()[0]
