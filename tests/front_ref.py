"""S0-S3 of the detector (gray conversion, decimation, adaptive threshold, connected components) stated in plain NumPy from
their definitions -- whole-array operations and a label propagation, none of the oracle's loops -- so that the oracle
(oracle/apriltag_oracle.c) and the HIP kernels (k_threshold.inc, k_seg.inc) are each held against an independent statement.
TEST INFRASTRUCTURE ONLY: sized for frames of a few ten thousand pixels."""
import numpy as np

TILE = 4          # pixels of a threshold tile's side
MIN_CONTRAST = 5  # max - min of a tile's 3x3 neighbourhood below this: "no contrast", 127


def bgr2gray(bgr):
    """(H, W, 3) uint8 BGR -> (H, W) uint8: 15-bit fixed point, round half up."""
    c = np.asarray(bgr).astype(np.int64)
    return ((3735 * c[..., 0] + 19235 * c[..., 1] + 9798 * c[..., 2] + 16384) >> 15).astype(np.uint8)


def decimate(gray, f):
    return np.ascontiguousarray(np.asarray(gray)[::f, ::f])


def _dilate(a, op):
    """3x3 neighbourhood reduction, the neighbourhood clamped into the grid (repeating an edge tile changes no min / max)."""
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    out = a.copy()
    for dy in range(3):
        for dx in range(3):
            out = op(out, p[dy:dy + h, dx:dx + w])
    return out


def tile_cuts(im):
    """(lo, hi) per full 4x4 tile after the 3x3 dilation, as int arrays of shape (sh // 4, sw // 4)."""
    sh, sw = im.shape
    tw, th = sw // TILE, sh // TILE
    t = np.asarray(im)[:TILE * th, :TILE * tw].reshape(th, TILE, tw, TILE).astype(np.int64)
    return _dilate(t.min(axis=(1, 3)), np.minimum), _dilate(t.max(axis=(1, 3)), np.maximum)


def threshold(im):
    """255 white, 0 black, 127 no contrast."""
    im = np.asarray(im)
    sh, sw = im.shape
    tw, th = sw // TILE, sh // TILE
    if tw == 0 or th == 0:
        return np.full((sh, sw), 127, np.uint8)
    lo, hi = tile_cuts(im)
    ty = np.minimum(np.arange(sh) // TILE, th - 1)[:, None]  # pixels beyond the last full tile use the nearest one
    tx = np.minimum(np.arange(sw) // TILE, tw - 1)[None, :]
    lo, hi = lo[ty, tx], hi[ty, tx]
    cut = lo + (hi - lo) // 2
    return np.where(hi - lo < MIN_CONTRAST, 127, np.where(im.astype(np.int64) > cut, 255, 0)).astype(np.uint8)


def links(th):
    """The undirected links of the threshold image as two index arrays: pixel (x, y) with 1 <= x <= sw - 2 links to an equal
    neighbour on its left, above it (y > 0) and, if white, above-left and above-right; 127 never links."""
    th = np.asarray(th)
    sh, sw = th.shape
    idx = np.arange(sh * sw).reshape(sh, sw)
    a, b = [], []

    def add(ys, xs, dy, dx, white_only):
        p = th[ys, xs]
        q = th[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
        m = (p == q) & ((p == 255) if white_only else (p != 127))
        a.append(idx[ys, xs][m])
        b.append(idx[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx][m])

    if sw >= 3:
        cols = slice(1, sw - 1)
        add(slice(0, sh), cols, 0, -1, False)
        if sh >= 2:
            rows = slice(1, sh)
            add(rows, cols, -1, 0, False)
            add(rows, cols, -1, -1, True)
            add(rows, cols, -1, 1, True)
    if not a:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(a), np.concatenate(b)


def components(th):
    """(labels, sizes), both (sh, sw) uint32: the label of a pixel is the smallest raster index of its component under
    links(); sizes holds the pixel count of a component at its label's pixel and 0 elsewhere (a 127 pixel is a component
    of one)."""
    th = np.asarray(th)
    sh, sw = th.shape
    n = sh * sw
    a, b = links(th)
    lab = np.arange(n)
    while True:  # hook every link's larger label under the smaller one, then shorten the chains; labels only ever fall
        la, lb = lab[a], lab[b]
        if np.array_equal(la, lb):
            break
        np.minimum.at(lab, la, lb)
        np.minimum.at(lab, lb, la)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    sizes = np.bincount(lab, minlength=n)
    return lab.reshape(sh, sw).astype(np.uint32), sizes.reshape(sh, sw).astype(np.uint32)


def front(frame, f):
    """All four products of one frame, (H, W) gray or (H, W, 3) BGR, at decimation f: gray, threshold, labels, sizes."""
    g = decimate(bgr2gray(frame) if np.asarray(frame).ndim == 3 else np.asarray(frame), f)
    th = threshold(g)
    lab, sz = components(th)
    return g, th, lab, sz
