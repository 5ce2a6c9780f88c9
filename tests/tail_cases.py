"""Deterministic frames on the edges of the per-quad tail (k_refine, k_homography, k_decode: k_refine.inc, k_decode.inc),
all of upright tags (family.grid, as in tag_sheet.py) on white, and a plain NumPy restatement, from the oracle's own
quads, of where each quad's edge probes, border samples and payload sites fall.

tagStandard41h12 has nine cells a side: ring 0 (outermost) holds data, ring 1 is black, ring 2 is the white border ring;
the detected quad is the boundary between rings 1 and 2 (black outside, white inside: reversed_border = 1).

tests/test_tail_cases.py checks under the oracle alone that every case reaches the edge it is named after;
tests/test_gpu_tail.py runs them on the device."""
import numpy as np

import oracle_lib as O
from tag_sheet import tag_sheet

PIX_EPS = 9.5367431640625e-07          # k_refine.inc
DEC_MAX_PROBES = 44                    # k_refine.inc: probes a lane parks; more take the step-by-step loop
TAIL_GRID_MIN = 8192                   # workgroups of k_refine / k_decode: max(8192, 64 B)
SITE_MARGIN = 0.25                     # px a site must lie outside the frame for rounding in H not to move it back
DARK = 40                              # black of the cropped tags: a probe or border sample outside the frame must not pass for a black pixel

# lost side -> a tag whose outer data ring holds at most one white bit on that side
CROP_IDS = {"left": 156, "right": 156, "top": 134, "bottom": 19}


def nprobe(f):
    """Probes per edge sample at decimate f: offsets -(f + 2) .. f + 2 in quarter pixels."""
    return 8 * (f + 1) + 9


def tag_image(family, tag_id, cell):
    return np.kron(family.grid(tag_id), np.ones((cell, cell), np.uint8)) * 255


def as_bgr(gray):
    """The same frame as BGR: equal channels convert back to exactly this gray."""
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


def lost_white_bits(family, tag_id, side):
    g = family.grid(tag_id)
    return int({"left": g[:, 0], "right": g[:, -1], "top": g[0], "bottom": g[-1]}[side].sum())


# ---- frames

def cropped(family, side, cell, kept, margin=None):
    """One tag on white, `margin` pixels from three frame edges; on `side` the frame ends inside ring 1, `kept` pixels from
    the quad's edge: ring 0 of that side (its data cells) and the rest of ring 1 are cut off.  Black is DARK, not 0: with
    0 a probe outside the frame counted as a pixel of ring 1, or an outside border sample counted as a black one, would
    change no sum."""
    margin = 3 * cell if margin is None else margin
    tag = np.where(tag_image(family, CROP_IDS[side], cell) > 0, 255, DARK).astype(np.uint8)
    n = tag.shape[0]
    f = np.full((n + 2 * margin, n + 2 * margin), 255, np.uint8)
    f[margin:margin + n, margin:margin + n] = tag
    cut = margin + 2 * cell - kept
    if side == "left":
        f = f[:, cut:]
    elif side == "right":
        f = f[:, :f.shape[1] - cut]
    elif side == "top":
        f = f[cut:]
    else:
        f = f[:f.shape[0] - cut]
    return np.ascontiguousarray(f)


# (decimate, cell, side, kept): every side at decimate 1 and 2, two sides at decimate 3, one at decimate 4.  The kept widths
# were picked so that the conditions of tests/test_tail_cases.py hold (a thinner ring 1 is no longer fitted as the quad's
# edge, behind a wider one no probe or border sample reaches the frame's edge).
CROPS = ((1, 8, "left", 2), (1, 8, "right", 2), (1, 8, "top", 2), (1, 8, "bottom", 2),
         (2, 12, "left", 3), (2, 8, "right", 3), (2, 12, "top", 3), (2, 8, "bottom", 2),
         (3, 12, "right", 4), (3, 12, "bottom", 3),
         (4, 16, "bottom", 3))
HIGH_SIDES = ("right", "bottom")  # crops whose probes can leave [0, w - 2] x [0, h - 1]; see probe_ends


def cropped_cases(family):
    """Every crop as a gray and as a BGR frame."""
    cases = []
    for dec, cell, side, kept in CROPS:
        g = cropped(family, side, cell, kept)
        for ch, fr in ((1, g), (3, as_bgr(g))):
            cases.append(dict(name="crop %s d%d c%d k%d %s" % (side, dec, cell, kept, "gray" if ch == 1 else "bgr"), frame=fr, gray=g,
                              decimate=dec, side=side, ids=[CROP_IDS[side]], maxhamming=2))
    return cases


SAMPLE_CELLS = {25: 64, 28: 68, 52: 128, 53: 132}  # cell -> edge samples of the tag's quad: 4 max(16, int(5 cell / 8))


def sample_count_cases(family):
    """One tag per frame whose quad has exactly one pass of 64 samples, one pass and 4, two passes, two passes and 4."""
    cases = []
    for cell, total in SAMPLE_CELLS.items():
        tag = tag_image(family, 7, cell)
        n, m = tag.shape[0], 2 * cell
        f = np.full((n + 2 * m, n + 2 * m), 255, np.uint8)
        f[m:m + n, m:m + n] = tag
        for dec in (1, 2):
            cases.append(dict(name="samples %d d%d" % (total, dec), frame=f, gray=f, decimate=dec, ids=[7], total=total))
    return cases


def three_tags(family):
    """Three tags for refine_edges=False."""
    return tag_sheet(family, 3 * 78 + 6, 84, 8, 6, ids=lambda k: 20 + k)


def flipped_cell(family):
    """Tag 33 with one interior payload cell flipped: hamming 1."""
    tag = tag_image(family, 33, 8)
    tag[32:40, 32:40] = 255 - tag[32:40, 32:40]  # cell (4, 4), the centre: a payload bit
    f = np.full((72 + 48, 72 + 48), 255, np.uint8)
    f[24:96, 24:96] = tag
    return f


def hollow_square(cell):
    """A black square of seven cells with a white core of five, the silhouette of rings 1 and 2 of a tag: its quad has the
    family's polarity (black outside, white inside) and so has its border, but no code is near the all-white payload."""
    s = np.zeros((7 * cell, 7 * cell), np.uint8)
    s[cell:6 * cell, cell:6 * cell] = 255
    return s


def outlined_square(cell):
    """A mid-gray square of seven cells inside a thin black outline, on white: the quad along the outline's inner side has
    the family's polarity (black outside, gray inside thresholds to white), but the border samples half a cell outside it
    land beyond the outline, on the white ground, brighter than the samples inside: the gray models find the wrong polarity."""
    t = max(2, cell // 3)
    s = np.zeros((7 * cell, 7 * cell), np.uint8)
    s[t:-t, t:-t] = 128
    return s


def _mixed_block(family, k, cell):
    """Block k of a mixed sheet, nine cells a side: a tag, an inverted tag, a hollow square or an outlined square."""
    if k % 4 == 0:
        return tag_image(family, k % 512, cell)
    if k % 4 == 1:
        return 255 - tag_image(family, k % 512, cell)
    b = np.full((9 * cell, 9 * cell), 255, np.uint8)
    b[cell:8 * cell, cell:8 * cell] = hollow_square(cell) if k % 4 == 2 else outlined_square(cell)
    return b


def mixed_sheet(family, width, height, cell, gap):
    """tag_sheet's layout with three blocks of four replaced (see _mixed_block)."""
    side = family.total_width * cell
    pitch = side + gap
    cols, rows = (width - gap) // pitch, (height - gap) // pitch
    img = np.full((height, width), 255, np.uint8)
    for k in range(cols * rows):
        y, x = gap + (k // cols) * pitch, gap + (k % cols) * pitch
        img[y:y + side, x:x + side] = _mixed_block(family, k, cell)
    return img


def skip_frame(family):
    """Decimate 2: two good tags, two inverted tags, two hollow and two outlined squares in one frame of eight blocks."""
    return mixed_sheet(family, 4 * 120 + 12, 2 * 120 + 12, 12, 12)


BATCH_W, BATCH_H, BATCH_N = 1280, 720, 20


def batch_frames(family):
    """The two distinct frames of the batch (a sheet of 464 tags of four-pixel cells; the same grid mixed) and the batch's
    order: they alternate."""
    a = tag_sheet(family, BATCH_W, BATCH_H, 4, 7)
    b = mixed_sheet(family, BATCH_W, BATCH_H, 4, 7)
    return [a, b], [i % 2 for i in range(BATCH_N)]


# ---- the oracle's quads and the restatement of the tail's sites

def oracle_quads(gray, family, f):
    """fit_quads' quads of a gray frame, their corners rescaled to full resolution as the tail does."""
    dec = O.decimate(gray, f)
    th = O.threshold(dec)
    lab, sz = O.connected_components(th)
    quads = O.fit_quads(dec, O.gradient_clusters(th, lab, sz), family, f, cap=8192)
    for q in quads:
        if f > 1:
            q["p"] = (q["p"] - 0.5) * f + 0.5
    return quads


def edge_samples(P, reversed_border):
    """(ns[4], x0, y0, nx, ny) of all samples of a quad with full-resolution corners P, edge by edge."""
    ns, X0, Y0, NX, NY = [], [], [], [], []
    for e in range(4):
        a, b = P[e], P[(e + 1) & 3]
        nx, ny = b[1] - a[1], -b[0] + a[0]
        mag = np.sqrt(nx * nx + ny * ny)
        nx, ny = nx / mag, ny / mag
        if reversed_border:
            nx, ny = -nx, -ny
        n = max(16, int(mag / 8))
        alpha = (1.0 + np.arange(n)) / (n + 1)
        ns.append(n)
        X0.append(alpha * a[0] + (1 - alpha) * b[0]); Y0.append(alpha * a[1] + (1 - alpha) * b[1])
        NX.append(np.full(n, nx)); NY.append(np.full(n, ny))
    return ns, np.concatenate(X0), np.concatenate(Y0), np.concatenate(NX), np.concatenate(NY)


def probe_ends(P, reversed_border, f):
    """ns[4], the pixels (n, 2, 2) of the first and the last probe of every sample, [sample, first / last, x / y], and the
    real coordinates they are truncated from.  The conversion is C's (int): a coordinate in (-1, 0) reads pixel 0, so at
    the frame's low edges a probe leaves only at -1 or below; an upright tag's edge that close to x = 0 or y = 0 leaves
    a ring 1 too thin to be fitted, and the left and top crops end with probes in (-1, 0) instead."""
    ns, x0, y0, nx, ny = edge_samples(P, reversed_border)
    t = float(f + 2)
    real = np.array([[x0 + s * t * nx + PIX_EPS, y0 + s * t * ny + PIX_EPS] for s in (-1.0, 1.0)]).transpose(2, 0, 1)
    return ns, np.trunc(real).astype(np.int64), real


def probes_leave(ends, w, h):
    """Samples with a probe outside [0, w - 2] x [0, h - 1], the region k_refine's unguarded probes need."""
    x, y = ends[:, :, 0], ends[:, :, 1]
    return ((x < 0) | (x > w - 2) | (y < 0) | (y > h - 1)).any(axis=1)


def homography(P):
    """H with H (-1,-1), (1,-1), (1,1), (-1,1) = P[0..3] and H[8] = 1 (np.linalg.solve: equal to the tail's to rounding)."""
    A, rhs = [], []
    for (x, y), (u, v) in zip(((-1, -1), (1, -1), (1, 1), (-1, 1)), P):
        A.append([x, y, 1, 0, 0, 0, -x * u, -y * u]); rhs.append(u)
        A.append([0, 0, 0, x, y, 1, -x * v, -y * v]); rhs.append(v)
    return np.append(np.linalg.solve(np.array(A, float), np.array(rhs, float)), 1.0)


def project(H, xy):
    xy = np.asarray(xy, float)
    z = H[6] * xy[:, 0] + H[7] * xy[:, 1] + H[8]
    return np.stack([(H[0] * xy[:, 0] + H[1] * xy[:, 1] + H[2]) / z, (H[3] * xy[:, 0] + H[4] * xy[:, 1] + H[5]) / z], axis=1)


def border_sites(family):
    """Tag-frame coordinates of the 8 x width_at_border border samples, and which belong to the "white" model."""
    wb = family.width_at_border
    pats = ((-0.5, 0.5, 0, 1, 1), (0.5, 0.5, 0, 1, 0), (wb + 0.5, .5, 0, 1, 1), (wb - 0.5, .5, 0, 1, 0),
            (0.5, -0.5, 1, 0, 1), (0.5, 0.5, 1, 0, 0), (0.5, wb + 0.5, 1, 0, 1), (0.5, wb - 0.5, 1, 0, 0))
    xy = [(2 * ((p[0] + i * p[2]) / wb - 0.5), 2 * ((p[1] + i * p[3]) / wb - 0.5)) for p in pats for i in range(wb)]
    return np.array(xy), np.array([p[4] for p in pats for i in range(wb)], bool)


def payload_sites(family):
    wb = family.width_at_border
    return np.stack([2 * ((family.bit_x + 0.5) / wb - 0.5), 2 * ((family.bit_y + 0.5) / wb - 0.5)], axis=1)


def border_outside(px, w, h, margin=SITE_MARGIN):
    """Border samples k_decode leaves out ((int) px < 0 or >= w, likewise y), by at least `margin`."""
    x, y = px[:, 0], px[:, 1]
    return (x <= -1 - margin) | (x >= w + margin) | (y <= -1 - margin) | (y >= h + margin)


def payload_outside(px, w, h, margin=SITE_MARGIN):
    """Payload sites whose four interpolation pixels do not all lie in the frame, by at least `margin`."""
    x, y = px[:, 0], px[:, 1]
    return (x < 0.5 - margin) | (x > w - 0.5 + margin) | (y < 0.5 - margin) | (y > h - 0.5 + margin)


def border_contrast(gray, H, family):
    """Mean gray under the "white" border samples minus that under the "black" ones (samples inside the frame): its sign,
    where it is far from 0, is the polarity k_decode's gray models find."""
    xy, white = border_sites(family)
    px = np.trunc(project(H, xy)).astype(np.int64)
    h, w = gray.shape
    ok = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
    v = gray[px[ok, 1], px[ok, 0]].astype(float)
    return v[white[ok]].mean() - v[~white[ok]].mean()


def quad_report(gray, family, f):
    """Per oracle quad of the frame: the rescaled corners, the sample counts, the samples whose probes leave the frame
    (`leave`) or have a negative coordinate (`low`: where it does not leave, it reads pixel 0), the refined corners, and the
    border and payload sites left out."""
    h, w = gray.shape
    out = []
    for q in oracle_quads(gray, family, f):
        ns, ends, real = probe_ends(q["p"], q["reversed_border"], f)
        R = O.refine_edges(gray, q["p"], q["reversed_border"], f)
        H = homography(R)
        out.append(dict(p=q["p"], reversed_border=q["reversed_border"], ns=ns, leave=probes_leave(ends, w, h),
                        low=(real < 0).any(axis=(1, 2)), refined=R, H=H,
                        border_out=border_outside(project(H, border_sites(family)[0]), w, h),
                        payload_out=payload_outside(project(H, payload_sites(family)), w, h)))
    return out


def undetected(gray, family, f, dets):
    """The oracle quads of the frame that no detection in `dets` sits on (a detection's centre lies within a pixel of the
    quad's refined centre H (0, 0))."""
    centres = np.array([d["center"] for d in dets]).reshape(-1, 2)
    out = []
    for r in quad_report(gray, family, f):
        c = project(r["H"], [(0.0, 0.0)])[0]
        if not len(centres) or np.abs(centres - c).max(axis=1).min() > 1.0:
            out.append(r)
    return out
