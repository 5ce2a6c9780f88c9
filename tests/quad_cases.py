"""Deterministic gray frames whose clusters sit on the quad fit's edges (k_quad.inc, size classes of k_cluster.inc).

Every case is a white shape on black, so its boundary cluster has the polarity tagStandard41h12 keeps (reversed border)
and runs through the whole fit.  The raw point count of a white w x h rectangle is 4 (w + h); taking a convex corner
pixel and its inward diagonal neighbour away lowers it by one, so every count is reachable.  A white rectangle in a
corner of the frame only has two sides inside the frame: 2 (w + h) - 4 points.

Shapes and positions are fixed: the floating-point values behind a maxima tie depend on where the shape lies.
tests/test_quad_cases.py checks every case under the oracle, so a case cannot drift off its edge unnoticed.

Frames are built at decimate 1; `scale=2` repeats every pixel 2 x 2, so that decimating by 2 gives the same image back.
"""
import numpy as np

import oracle_lib as O
from aprilslam_amd import synth

CLASS_CAPS = (128, 256, 512, 1024)  # CLASS0_CAP .. CLASS3_CAP of asl_common.h
W, H = 1280, 720                    # edge frames
LIMIT_WH = 64                       # the small frames of the upper limit: L = 3 (2 sw + 2 sh) = 768
TAG_ROWS = 180                      # the tag strip at the bottom of the edge frames


def size_class(count):
    for c, cap in enumerate(CLASS_CAPS):
        if count <= cap:
            return c
    return len(CLASS_CAPS)


def upper_limit(sw, sh):
    return 3 * (2 * sw + 2 * sh)


def rect(w, h, trims=0):
    """White w x h mask; `trims` (0..4) convex corners lose their corner pixel and its inward diagonal: -1 point each."""
    m = np.ones((h, w), np.uint8)
    for x, y, dx, dy in [(0, 0, 1, 1), (w - 1, 0, -1, 1), (0, h - 1, 1, -1), (w - 1, h - 1, -1, -1)][:trims]:
        m[y, x] = 0
        m[y + dy, x + dx] = 0
    return m


def rect_for(count):
    """A near-square rect() mask with exactly `count` raw points (count >= 40)."""
    n = -(-count // 4)
    return rect(n // 2, n - n // 2, 4 * n - count)


def notched(w, h, notches):
    """w x h rectangle with square notches of the given sizes cut from its corners (tl, tr, bl, br): more corners."""
    m = np.ones((h, w), np.uint8)
    for k, n in enumerate(notches):
        if n:
            m[slice(0, n) if k < 2 else slice(h - n, h), slice(0, n) if k % 2 == 0 else slice(w - n, w)] = 0
    return m


def comb(ntooth, tooth_len, longer, trims, tooth_w=2, tooth_gap=3, base_w=56, base_h=6):
    """A bar with teeth hanging from it, a boundary far longer than its box: the first `longer` teeth are one pixel longer."""
    m = np.zeros((base_h + tooth_len + 1, base_w), np.uint8)
    m[:base_h] = 1
    for k in range(ntooth):
        x = 4 + k * (tooth_w + tooth_gap)
        m[base_h:base_h + tooth_len + (1 if k < longer else 0), x:x + tooth_w] = 1
    bh = base_h - 1
    for x, y, dx, dy in [(0, 0, 1, 1), (base_w - 1, 0, -1, 1), (0, bh, 1, -1), (base_w - 1, bh, -1, -1)][:trims]:
        m[y, x] = 0
        m[y + dy, x + dx] = 0
    return m


def _paste(img, mask, x, y):
    img[y:y + mask.shape[0], x:x + mask.shape[1]][mask > 0] = 255
    ys, xs = np.nonzero(mask)
    return int(x + xs[0]), int(y + ys[0])  # the shape's first pixel in raster order: its component's label


def _tag_strip(seed):
    rng = np.random.default_rng(seed)
    tags = synth.random_scene(W, TAG_ROWS, 4, rng)
    frame, _ = synth.render_frame(W, TAG_ROWS, tags, 18.0, rng=rng)
    return O.bgr2gray(frame)


def _scaled(frames, cases, scale):
    if scale != 1:
        frames = frames.repeat(scale, axis=1).repeat(scale, axis=2)
    return np.ascontiguousarray(frames), cases


def edge_frames(scale=1):
    """Two 1280 x 720 gray frames (x scale) and their cases: dicts of name, frame, (x, y) of a pixel of the shape in the
    decimated image, the raw point count and what the maxima stage must see ("maxima": None, 4, 10, ">10" or "tie")."""
    frames = np.zeros((2, H, W), np.uint8)
    cases = []

    def put(f, name, mask, x, y, count=None, maxima=None):
        px, py = _paste(frames[f], mask, x, y)
        cases.append(dict(name=name, frame=f, x=px, y=py, count=count, maxima=maxima))

    # frame 0: the size-class edges.  The two top corners: a rectangle there has only two sides in the frame
    m = rect(7, 7)
    put(0, "floor 24", m, 0, 0, 24)
    m = rect(7, 7)
    m[6, 0] = 0; m[5, 1] = 0  # the inner corner of the mirrored corner rectangle: -1
    put(0, "floor 23", m[:, ::-1].copy(), W - 7, 0, 23)
    x = 30
    for count in (128, 129, 256, 257, 512, 513, 1024, 1025):
        m = rect_for(count)
        put(0, "count %d" % count, m, x, 20, count)
        x += m.shape[1] + 40
    put(0, "class 4 2048", rect(256, 256), 30, 190, 2048, "tie")
    put(0, "class 4 2599", rect(400, 250, 1), 330, 190, 2599, "tie")
    put(0, "class 4 comb", comb(10, 70, 3, 2, tooth_w=4, tooth_gap=8, base_w=130, base_h=30), 780, 190, 3450, ">10")
    frames[0, H - TAG_ROWS:] = _tag_strip(1)

    # frame 1: the maxima edges
    put(1, "4 maxima class 0", rect(12, 16), 30, 30, 112, 4)
    put(1, "4 maxima class 1", rect(30, 32), 90, 36, 248, 4)
    put(1, "10 maxima", notched(40, 40, (10, 10, 10, 0)), 170, 30, 320, 10)
    put(1, "12 maxima class 1", notched(30, 30, (8, 8, 8, 8)), 260, 30, 240, ">10")
    put(1, "12 maxima class 2", notched(60, 60, (15, 15, 15, 15)), 340, 30, 480, ">10")
    put(1, "tie class 2", notched(31, 87, (7, 0, 7, 6)), 450, 30, 472, "tie")
    put(1, "tie class 3", rect(87, 97), 530, 30, 736, "tie")
    put(1, "tie class 3 notched", notched(76, 81, (0, 20, 23, 6)), 670, 30, 628, "tie")
    put(1, "maxima class 4", notched(300, 200, (40, 30, 20, 60)), 30, 220, 2000, ">10")
    frames[1, H - TAG_ROWS:] = _tag_strip(2)
    return _scaled(frames, cases, scale)


def limit_frames(scale=1):
    """Two 64 x 64 frames (x scale), each with one comb: exactly the upper limit L = 768 points, and L + 1 (dropped)."""
    frames = np.zeros((2, LIMIT_WH, LIMIT_WH), np.uint8)
    cases = []
    for f, (args, count) in enumerate((((3, 43, 1, 0), 768), ((3, 43, 2, 3), 769))):
        px, py = _paste(frames[f], comb(*args), 4, 4)
        cases.append(dict(name="limit %d" % count, frame=f, x=px, y=py, count=count, maxima=None))
    return _scaled(frames, cases, scale)


def oracle_stages(gray, family, decimate):
    """The oracle's S1..S5 on one gray frame: decimated image, labels, boundary points, per-cluster maxima records."""
    dec = O.decimate(gray, decimate)
    th = O.threshold(dec)
    lab, sz = O.connected_components(th)
    pts = O.gradient_clusters(th, lab, sz)
    return dec, lab, pts, O.quad_maxima(dec, pts, family, decimate)


def case_records(frames, cases, family, decimate):
    """Each case's oracle maxima record (MAXIMA_DTYPE), found through its shape's component label."""
    out = []
    per_frame = {}
    for c in cases:
        if c["frame"] not in per_frame:
            per_frame[c["frame"]] = oracle_stages(frames[c["frame"]], family, decimate)
        dec, lab, pts, st = per_frame[c["frame"]]
        label = int(lab[c["y"], c["x"]])
        mine = st[((st["cluster"] >> np.uint64(32)) == label) | ((st["cluster"] & np.uint64(0xFFFFFFFF)) == label)]
        assert len(mine) == 1, (c["name"], len(mine))
        out.append(mine[0])
    return out


def grid_texture(w, h, pitch_x, pitch_y, trims=0):
    """A 1280 x 720 frame tiled with white w x h rectangles (rect(w, h, trims)): one cluster of 4 (w + h) - trims points each."""
    f = np.zeros((H, W), np.uint8)
    m = rect(w, h, trims)
    for y in range(6, H - h - 6, pitch_y):
        for x in range(6, W - w - 6, pitch_x):
            f[y:y + h, x:x + w][m > 0] = 255
    return f


def batch_textures():
    """Distinct 1280 x 720 frames for the batch-scale test at decimate 1, each dense in one size class, and a tag scene."""
    rng = np.random.default_rng(5)
    tags = synth.random_scene(W, H, 12, rng)
    scene, _ = synth.render_frame(W, H, tags, 18.0, rng=rng)
    return {
        0: grid_texture(10, 10, 18, 18),         # 80 points
        1: grid_texture(17, 16, 26, 26, 1),      # 131
        2: grid_texture(33, 32, 44, 44, 2),      # 258
        3: grid_texture(120, 10, 132, 20, 3),    # 517
        4: grid_texture(250, 12, 262, 22, 1),    # 1047
        "tags": O.bgr2gray(scene),
    }
