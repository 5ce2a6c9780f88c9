"""Deterministic frames on the edges of S0-S3: decimation (k_decimate2_tiles / k_decimate_rest / k_decimate_minmax,
k_threshold.inc), the tile cut and the threshold (k_tile_cut, seg_threshold_tile) and the labelling (k_seg_tile,
k_seg_tile_dense, k_seg_border, k_seg_roots; k_seg.inc).  Every case is a dict with a name, a frame ((H, W) gray or
(H, W, 3) BGR uint8) and the decimation factor "f"; what else it carries is said at its generator.

tests/test_front_cases.py proves on the CPU that every frame reaches the edge it is named after, tests/test_gpu_front.py
holds the kernels to the oracle and to tests/front_ref.py on them.  The labelling works on words of 64 pixels and tiles of
32 rows (one wavefront per 64 x 32 tile), the tile cut on blocks of 4 x 4 threshold tiles (16 x 16 pixels)."""
import functools

import numpy as np

import front_ref
from seg_cases import DARK, LIGHT

WORD, ROWS = 64, 32   # pixels of a word, rows of a labelling tile (SEG_TH)
SEG_CAP = 512         # runs, and links, the common labelling launch holds per tile (k_seg.inc)
FACTORS = (1, 2, 3, 4, 8)


# ---------------------------------------------------------------------------------------------- counting, as k_seg_tile does
def _shl(a):
    """bit x <- bit x - 1 (the kernel's M << 1)"""
    out = np.zeros_like(a)
    out[..., 1:] = a[..., :-1]
    return out


def _shr(a):
    """bit x <- bit x + 1 (the kernel's M >> 1)"""
    out = np.zeros_like(a)
    out[..., :-1] = a[..., 1:]
    return out


def join_mask(x0, sw):
    """seg_join_mask: the pixels of word x0 / 64 that may initiate links, 1 <= x0 + x <= sw - 2, as 64 booleans."""
    x = x0 + np.arange(WORD)
    return (x >= 1) & (x <= sw - 2)


def tile_counts(th):
    """{(word column, tile row): (runs, links)} of every 64 x 32 labelling tile of a threshold image, counted as
    k_seg_tile counts them: run starts of both colours under the join mask (seg_starts), links to the row above inside
    the tile as seg_links states them (up: one per stretch; up-left where up does not connect; up-right unless up connects
    and x + 1 joins x above; the diagonals are white's alone)."""
    sh, sw = th.shape
    out = {}
    for ty in range((sh + ROWS - 1) // ROWS):
        for wx in range((sw + WORD - 1) // WORD):
            J = join_mask(wx * WORD, sw)
            runs = nlinks = 0
            for colour in (255, 0):
                M = np.zeros((ROWS, WORD), bool)
                part = th[ty * ROWS:(ty + 1) * ROWS, wx * WORD:(wx + 1) * WORD] == colour
                M[:part.shape[0], :part.shape[1]] = part
                Mp = np.zeros_like(M)
                Mp[1:] = M[:-1]
                runs += int((M & ~(_shl(M) & J)).sum())
                U = M & Mp & J
                nlinks += int((U & ~_shl(U)).sum())
                if colour == 255:
                    nlinks += int((M & J & _shl(Mp) & ~Mp).sum())
                    nlinks += int((M & J & _shr(Mp) & ~(Mp & _shr(J))).sum())
            out[(wx, ty)] = (runs, nlinks)
    return out


def dense_tiles(th):
    """Tiles the common launch hands to k_seg_tile_dense: more than SEG_CAP runs or links."""
    return sum(1 for r, l in tile_counts(th).values() if r > SEG_CAP or l > SEG_CAP)


# ------------------------------------------------------------------------------------------------------------ drawing helpers
def noise(shape, seed):
    """seeded per-pixel random bytes"""
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def block_texture(sw, sh, seed):
    """the 4 x 4-block texture of seg_cases.sizes(): one block in six white"""
    blocks = np.random.default_rng(seed).random(((sh + 3) // 4, (sw + 3) // 4)) < 1 / 6
    return np.where(blocks.repeat(4, axis=0).repeat(4, axis=1)[:sh, :sw], LIGHT, DARK).astype(np.uint8)


def _or3(a):
    p = np.pad(a, 1, mode="edge")
    h, w = a.shape
    out = np.zeros_like(a)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def salt(frame):
    """Makes the threshold of a DARK / LIGHT drawing exactly gray > 127: wherever the 3 x 3 neighbourhood of a 4 x 4 tile
    holds one value only, a tile of a 3-tile lattice nearby gets one pixel of the other value at its offset (2, 1).  That
    pixel's eight neighbours lie inside its uniform tile, so it is a component of its own, touches nothing that is drawn,
    sits on no word or row seam (x = 2 mod 4, y = 1 mod 4) and cuts nothing apart (the ring around it stays closed)."""
    sh, sw = frame.shape
    tw, th = sw // 4, sh // 4
    t = frame[:4 * th, :4 * tw].reshape(th, 4, tw, 4)
    light, dark = (t == LIGHT).any(axis=(1, 3)), (t == DARK).any(axis=(1, 3))
    need = ~(_or3(light) & _or3(dark))
    ly = (np.arange(th) % 3 == 1) | ((np.arange(th) == th - 1) & ((th - 1) % 3 == 0))
    lx = (np.arange(tw) % 3 == 1) | ((np.arange(tw) == tw - 1) & ((tw - 1) % 3 == 0))
    pick = _or3(need) & ly[:, None] & lx[None, :] & ~(light & dark)
    for ty, tx in zip(*np.nonzero(pick)):
        frame[4 * ty + 1, 4 * tx + 2] = DARK if light[ty, tx] else LIGHT
    return frame


def binary(th_or_gray):
    """what the threshold of a salted DARK / LIGHT drawing must be"""
    return np.where(np.asarray(th_or_gray) > 127, 255, 0).astype(np.uint8)


def _case(name, frame, f=1, **more):
    return dict(name=name, frame=np.ascontiguousarray(frame, dtype=np.uint8), f=f, **more)


# ================================================================================================ A. layout and decimation
RESIDUE_SIZES = ((16, 13), (17, 14), (18, 15), (19, 12))  # (sw, sh): every residue of sw mod 4 and of sh mod 4


def decimation():
    """Seeded random bytes, gray and BGR.  Factors 2 (k_decimate2_tiles + k_decimate_rest) and 3 (k_decimate_minmax) at the
    four RESIDUE_SIZES, the input width alternately a multiple of f and one more than a multiple; factors 1, 4 and 8 at one
    size each whose width and height are no multiple of f."""
    cases = []
    for f in (2, 3):
        for k, (sw, sh) in enumerate(RESIDUE_SIZES):
            w = sw * f if k % 2 == 0 else (sw - 1) * f + 1
            h = (sh - 1) * f + 1 if k % 2 == 0 else sh * f
            for ch in (1, 3):
                cases.append(_case("decimate %d: %dx%d ch %d" % (f, w, h, ch), noise((h, w) if ch == 1 else (h, w, 3), 1000 + 10 * f + k), f, dec=(sw, sh)))
    for f, w, h in ((1, 21, 14), (4, 71, 50), (8, 133, 75)):
        for ch in (1, 3):
            cases.append(_case("decimate %d: %dx%d ch %d" % (f, w, h, ch), noise((h, w) if ch == 1 else (h, w, 3), 1100 + f), f,
                               dec=(1 + (w - 1) // f, 1 + (h - 1) // f)))
    return cases


def corner_colours():
    """The eight 0 / 255 corners of the BGR cube as 8 x 8 blocks, 32 x 16; at decimate 1 and 2."""
    f = np.zeros((16, 32, 3), np.uint8)
    for k in range(8):
        f[8 * (k // 4):8 * (k // 4) + 8, 8 * (k % 4):8 * (k % 4) + 8] = [255 * (k & 1), 255 * ((k >> 1) & 1), 255 * ((k >> 2) & 1)]
    return [_case("corner colours, decimate %d" % d, f, d) for d in (1, 2)]


def padded_layouts():
    """(name, f, channels, frames (3, H, W[, 3])) of the batches that go through detect_device with padded rows and frames."""
    return [("padded BGR, decimate 2", 2, 3, noise((3, 29, 37, 3), 1201)), ("padded gray, decimate 2", 2, 1, noise((3, 29, 37), 1202)),
            ("padded BGR, decimate 3", 3, 3, noise((3, 31, 40, 3), 1203))]


def pad_batch(frames, ch):
    """The batch laid out with stride = w ch + 5 and frame_pitch = stride h + 11, the padding filled with alternating
    0 / 255 (a byte read from it would change a gray value or a tile extremum).  Returns (bytes, stride, frame_pitch)."""
    B, h, w = frames.shape[:3]
    stride = w * ch + 5
    pitch = stride * h + 11
    buf = (255 * (np.arange(B * pitch) & 1)).astype(np.uint8)
    for b in range(B):
        rows = buf[b * pitch:b * pitch + stride * h].reshape(h, stride)
        rows[:, :w * ch] = frames[b].reshape(h, w * ch)
    return buf, stride, pitch


def smallest_frames():
    """8 x 8 at decimate 1, 2, 3 and 8, and 9 x 9 at decimate 8 (gray and BGR): for the last three the decimated image
    (3 x 3, 1 x 1, 2 x 2) is smaller than a tile, everything is 127 and k_tile_cut is not launched."""
    cases = []
    for n, f in ((8, 1), (8, 2), (8, 3), (8, 8), (9, 8)):
        for ch in (1, 3):
            s = 1 + (n - 1) // f
            cases.append(_case("smallest %dx%d decimate %d ch %d" % (n, n, f, ch), noise((n, n) if ch == 1 else (n, n, 3), 1300 + 10 * n + f), f, dec=(s, s)))
    return cases


# ================================================================================================================ B. threshold
def contrast_floor():
    """32 rows on a uniform ground, 32 wide (eight tiles: k_tile_cut's packed path) and 36 wide (nine: the pixel's tile is the
    last block's, cut byte by byte); "expect" lists ((x, y), value of the threshold image), "blank" says that all is 127.
    The pixels sit in the tile of column X = 13 or 33."""
    c = []
    for sw, X in ((32, 13), (36, 33)):
        def add(name, ground, pixels):
            """pixels: ((x, y), gray value, threshold value); none is coloured if the first one is not"""
            f = np.full((32, sw), ground, np.uint8)
            for (x, y), v, _ in pixels:
                f[y, x] = v
            blank = pixels[0][2] == 127
            expect = [] if blank else [(p, t) for p, _, t in pixels] + [((X - 1, 12), 0), ((0, 0), 127)]  # + ground in the pixel's tile, a tile far away
            c.append(_case("%s, %d wide" % (name, sw), f, blank=blank, expect=expect))
        add("floor: 104 on 100", 100, [((X, 13), 104, 127)])
        add("floor: 105 on 100", 100, [((X, 13), 105, 255)])
        # max - min = 10: the cut is 105; a pixel equal to it is black, one above it white
        add("cut: equal is black", 100, [((X, 13), 110, 255), ((X + 1, 13), 105, 0), ((X, 14), 106, 255)])
        # max - min = 11: (max - min) / 2 takes the floor, the cut is 105 again
        add("cut: odd difference", 100, [((X, 13), 111, 255), ((X + 1, 13), 105, 0), ((X, 14), 106, 255)])
        add("cut: 0 / 255", 0, [((X, 13), 255, 255), ((X + 1, 13), 127, 0), ((X, 14), 128, 255)])
        # the largest cut there is, 252, next to the kernel's 255 = "no contrast"
        add("cut: 252", 250, [((X, 13), 255, 255), ((X + 1, 13), 253, 255), ((X, 14), 252, 0)])
    return c


REACH = (  # (tiles across, tiles down, [(tile x, tile y) of the one off-ground pixel])
    (9, 9, [(0, 0), (8, 0), (0, 8), (8, 8), (3, 1), (4, 1), (1, 3), (1, 4), (3, 3), (4, 4)]),  # corners; both sides of the block seams 3|4
    (8, 5, [(7, 2)]), (10, 5, [(9, 2)]), (11, 5, [(10, 2), (8, 4)]),                               # last tile column, tw mod 4 = 0, 2, 3 (1: above)
    (4, 4, [(0, 0), (3, 3)]),                                                                      # one block, first and last at once
    (3, 6, [(2, 5)]), (6, 3, [(5, 2)]), (2, 2, [(1, 0)]),                                          # tw < 4, th < 4, both
)


def dilation_reach():
    """One pixel of 200 on ground 100 in tile (tx, ty) of a frame of tw x th whole tiles: exactly the tiles of its 3 x 3
    neighbourhood, clamped at the borders, are coloured.  "box" = (x0, y0, x1, y1), inclusive, of the coloured pixels."""
    cases = []
    for tw, th, places in REACH:
        for tx, ty in places:
            f = np.full((4 * th, 4 * tw), 100, np.uint8)
            f[4 * ty + 2, 4 * tx + 1] = 200
            box = (4 * max(tx - 1, 0), 4 * max(ty - 1, 0), 4 * min(tx + 1, tw - 1) + 3, 4 * min(ty + 1, th - 1) + 3)
            cases.append(_case("reach: %dx%d tiles, pixel in tile (%d, %d)" % (tw, th, tx, ty), f, box=box, tiles=(tw, th), at=(tx, ty)))
    return cases


LEFTOVER_SIZES = ((65, 37), (66, 38), (67, 39))  # sw mod 4, sh mod 4 = 1, 2, 3


def leftovers():
    """Ground 100.  "alone": a bright pixel in the leftover columns, one in the leftover rows: no full tile sees them, all
    is 127.  "beside": the last full tiles hold a pixel of 200, so their cut (150) thresholds the leftover pixels next to
    them: 151 is white, 150 black."""
    cases = []
    for sw, sh in LEFTOVER_SIZES:
        tw, th = sw // 4, sh // 4
        f = np.full((sh, sw), 100, np.uint8)
        f[10, sw - 1] = 200
        f[sh - 1, 10] = 200
        cases.append(_case("leftover %dx%d: alone" % (sw, sh), f, blank=True, expect=[]))
        g = np.full((sh, sw), 100, np.uint8)
        g[10, 4 * tw - 2] = 200   # in the last tile column
        g[10, sw - 1] = 151
        g[11, 4 * tw] = 150
        g[4 * th - 2, 10] = 200   # in the last tile row
        g[sh - 1, 10] = 151
        g[4 * th, 11] = 150
        cases.append(_case("leftover %dx%d: beside a tile with contrast" % (sw, sh), g, blank=False,
                           expect=[((sw - 1, 10), 255), ((4 * tw, 11), 0), ((4 * tw - 2, 10), 255), ((10, sh - 1), 255), ((11, 4 * th), 0), ((sw - 1, 9), 0),
                                   ((30, 20), 127)]))
    return cases


SEGMENT_SIZES = ((16, 16), (17, 16), (63, 31), (64, 32), (65, 33), (79, 49), (127, 31), (129, 65))  # (sw, sh)


def segments():
    """seg_threshold_tile's 16-pixel segments, the 64-pixel word and the two 16-row halves: every size once with per-pixel
    noise ("dense": tiles of 63 x 31 and more go to k_seg_tile_dense) and once with the block texture (common launch)."""
    cases = []
    for k, (sw, sh) in enumerate(SEGMENT_SIZES):
        cases.append(_case("segments %dx%d noise" % (sw, sh), noise((sh, sw), 1400 + k), kind="noise"))
        for seed in range(1450 + k, 3450, 100):  # the first seed that colours the last column and the last row
            f = block_texture(sw, sh, seed)
            th = front_ref.threshold(f)
            if (th[:, -1] != 127).any() and (th[-1] != 127).any():
                break
        cases.append(_case("segments %dx%d blocks" % (sw, sh), f, kind="blocks"))
    return cases


# ================================================================================================================ C. labelling
CW, CH = 80, 44  # the single-contact frames


def _blob(p, d, side):
    """A pixel p, a stalk of two more pixels in direction d and a 6 x 6 body behind it that extends from the stalk's line
    towards `side` (for a vertical stalk: -1 left, +1 right; a horizontal stalk's body is centred on it)."""
    (x, y), (dx, dy) = p, d
    cells = [(x + k * dx, y + k * dy) for k in range(3)]
    if dx == 0:
        xs = range(x, x + 6) if side > 0 else range(x - 5, x + 1)
        cells += [(i, y + k * dy) for k in range(3, 9) for i in xs]
    else:
        cells += [(x + k * dx, j) for k in range(3, 9) for j in range(y - 3, y + 3)]
    return cells


CONTACT_PLACES = {  # kind -> {place: b}, b the lower / right pixel of the pair
    "h": {"inside": (20, 12), "word seam": (64, 12), "corner, row 31": (64, 31), "corner, row 32": (64, 32)},
    "v": {"inside": (20, 12), "row seam": (20, 32), "corner, column 63": (63, 32), "corner, column 64": (64, 32)},
    "up-left": {"inside": (20, 12), "word seam": (64, 12), "row seam": (20, 32), "corner": (64, 32)},
    "up-right": {"inside": (20, 12), "word seam": (63, 12), "row seam": (20, 32), "corner": (63, 32)},
}
_PAIR_A = {"h": (-1, 0), "v": (0, -1), "up-left": (-1, -1), "up-right": (1, -1)}  # a - b


def single_contacts():
    """Two blobs whose only contact is the pixel pair a, b, in white on a dark ground and in black on a light one.  b is the
    pixel that initiates the link: to its left (h), up (v), up-left or up-right.  Carries a, b, the blobs' cells A and B,
    the colour and whether the blobs must merge (white always; black through h and v only)."""
    cases = []
    for white in (True, False):
        for kind, places in CONTACT_PLACES.items():
            for place, b in places.items():
                a = (b[0] + _PAIR_A[kind][0], b[1] + _PAIR_A[kind][1])
                if kind == "h":
                    A, B = _blob(a, (-1, 0), 0), _blob(b, (1, 0), 0)
                else:
                    s = 1 if kind == "up-right" else -1
                    A, B = _blob(a, (0, -1), s), _blob(b, (0, 1), -s)
                f = np.full((CH, CW), DARK if white else LIGHT, np.uint8)
                for x, y in A + B:
                    f[y, x] = LIGHT if white else DARK
                cases.append(_case("contact: %s %s, %s" % ("white" if white else "black", kind, place), salt(f), a=a, b=b, A=A, B=B, white=white,
                                   kind=kind, place=place, merges=white or kind in ("h", "v")))
    return cases


def last_column():
    """White at (sw - 2, y), (sw - 2, y - 1) and (sw - 1, y - 1) for y = 12 (inside a tile) and y = 32 (row seam): pixel sw - 1
    joins only through the up-right diagonal, which "up" does not make redundant there.  sw = 64, 65, 66: column sw - 1 is
    bit 63 of its word, bit 0 of the next word, or bit 1.  A stalk below (sw - 2, y) makes the component 8 pixels."""
    cases = []
    for sw in (64, 65, 66):
        f = np.full((CH, sw), DARK, np.uint8)
        for y in (12, 32):
            f[y - 1:y + 6, sw - 2] = LIGHT
            f[y - 1, sw - 1] = LIGHT
        cases.append(_case("last column, sw = %d" % sw, salt(f), sites=[(sw, 12), (sw, 32)]))
    return cases


BAR_ROWS = range(2, 42)  # 40 rows, across row 32


def border_columns():
    """66 x 44: a bar in column 0 and one in column 65, white on dark and black on light.  Beside the left bar, column 1 has
    the bar's colour in rows 10 and 11; beside the right bar, column 64 has it in row 21.  "groups": the components that
    hold more than one pixel, as sets of (x, y); every other bar pixel is a component of one."""
    cases = []
    for white in (True, False):
        sw = 66
        f = np.full((CH, sw), DARK if white else LIGHT, np.uint8)
        v = LIGHT if white else DARK
        for y in BAR_ROWS:
            f[y, 0] = f[y, sw - 1] = v
        f[10, 1] = f[11, 1] = f[21, sw - 2] = v
        if white:  # (1, 10) reaches (0, 9) up-left, (1, 11) reaches (0, 10); (64, 21) reaches (65, 20) up-right
            groups = [{(0, 9), (0, 10), (0, 11), (1, 10), (1, 11)}, {(64, 21), (65, 20)}]
        else:      # a black pixel of the last column joins nothing
            groups = [{(0, 10), (0, 11), (1, 10), (1, 11)}]
        cases.append(_case("border columns, %s" % ("white" if white else "black"), salt(f), white=white, groups=groups))
    return cases


LW, LH = 192, 96  # 3 words x 3 row blocks


def _spiral(sw, sh, pitch):
    f = np.full((sh, sw), DARK, np.uint8)
    x0, y0, x1, y1 = 2, 1, sw - 3, sh - 2
    x, y = x0, y0
    f[y, x] = LIGHT
    while True:
        moved = False
        for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            while True:  # run on until the frame's margin or a white pixel within `pitch` pixels ahead
                nx, ny = x + dx, y + dy
                if not (x0 <= nx <= x1 and y0 <= ny <= y1):
                    break
                ahead = [(x + k * dx, y + k * dy) for k in range(1, pitch + 1)]
                if any(x0 <= ax <= x1 and y0 <= ay <= y1 and f[ay, ax] == LIGHT for ax, ay in ahead):
                    break
                x, y = nx, ny
                f[y, x] = LIGHT
                moved = True
        if not moved:
            return f


def _comb(sw, sh):
    """Groups of six one-pixel teeth on a 2-pixel pitch, one group per word seam (three teeth on either side of it), from
    row 2 down to a spine in row sh - 3: few enough runs per tile for the common launch."""
    f = np.full((sh, sw), DARK, np.uint8)
    for g0 in range(58, sw - 4, WORD):
        f[2:sh - 3, g0:min(g0 + 12, sw - 4):2] = LIGHT
    f[sh - 3, 4:sw - 4] = LIGHT
    return f


def long_components():
    """192 x 96.  "spiral": a one-pixel white spiral of pitch 10 from (2, 1) inwards -- one white component, and its
    complement, one black component that holds every black pixel but the last column's, each of which is alone.  "comb" /
    "comb, mirrored": teeth that meet only in the spine of row 93 / row 2: until the seams are merged every tile above
    (below) holds a root per tooth.  Carries "white" = (size, root) of the one white component and "black" of the black one."""
    cases = []
    for name, f in (("spiral", _spiral(LW, LH, 10)), ("comb", _comb(LW, LH)), ("comb, mirrored", _comb(LW, LH)[::-1].copy())):
        nwhite = int((f == LIGHT).sum())
        root = int(np.flatnonzero(f.ravel() == LIGHT)[0])
        f = salt(f)  # white pixels only: the ground is dark
        nblack = int((f == DARK).sum()) - LH
        cases.append(_case(name, f, white=(nwhite, root), black=(nblack, 0)))
    return cases


SW_SEAM, SH_SEAM = 128, 44


def _seam_frames(sw, sh, x0, x1, pitch=5):
    """Four drawings whose features span columns x0 .. x1 - 1 (across word seam 64) and rows 2 .. sh - 3 (across row 32)."""
    rows = slice(2, sh - 2)
    band_w = np.full((sh, sw), DARK, np.uint8)
    band_w[rows, x0:x1] = LIGHT
    band_b = np.full((sh, sw), LIGHT, np.uint8)
    band_b[rows, x0:x1] = DARK
    rungs = np.full((sh, sw), DARK, np.uint8)
    rungs[2:sh - 2:2, x0:x1] = LIGHT
    stairs = np.full((sh, sw), DARK, np.uint8)
    for y in range(2, sh - 2):
        for c in range(x0 - sh, x1, pitch):  # 3-pixel steps that move one column per row, a stripe every `pitch` columns
            for x in range(c + y, c + y + 3):
                if x0 <= x < x1:
                    stairs[y, x] = LIGHT
    return [("white band", band_w), ("black band", band_b), ("rungs", rungs), ("stairs", stairs)]


def seam_pairs():
    """128 x 44, k_seg_border's word-seam lanes leave a link to the row above when that row holds the same pair of roots.
    Bands: the same pair in all 40 rows, across row 32.  "rungs": one-pixel white lines in every second row, each a
    component of its own, so no two rows hold the same white pair.  "stairs": diagonal white stripes of 3-pixel steps: a
    stripe crosses the seam in two consecutive rows (the same pair twice), the next stripe three rows on."""
    return [_case("seam pairs: " + n, salt(f)) for n, f in _seam_frames(SW_SEAM, SH_SEAM, 50, 80)]


def label_batch():
    """Three different frames of 130 x 40 (three words, 80 seam rows a frame: the 64-lane seam workgroups straddle word
    columns and frames), their features across both word seams and up to the last column."""
    fr = _seam_frames(130, 40, 50, 130, pitch=16)  # 80 columns of stripes: a wider pitch keeps the tiles in the common launch
    return [_case("batch: " + n, salt(f)) for n, f in (fr[0], fr[2], fr[3])]


# ---- table capacity
CAP_W, CAP_H = 192, 64
CAP_TILE = (1, 0)  # the tile under test: word column 1, tile row 0; ordinary tiles on its left, right and below


def _capacity_frame(stripe_cols, stripe_rows, part, comb_rows, comb_cols, comb_part, bars, tweak):
    """Dark ground.  In the tile under test (columns 64 .. 127, rows 0 .. 31): one-pixel vertical stripes (white at even
    offsets) over `stripe_cols` columns from column 65 and `stripe_rows` rows from row 1, `part` columns more in the row
    below; or rows alternating W.W.W... and all-white over `comb_cols` columns (`comb_rows` rows, then `comb_part` pixels
    of one more all-white row); `bars` vertical 2-pixel bars (one link each) and `tweak` single pixels in column 64 (one
    run each).  A white line in row 20 from column 40 to 150 and one in column 100 from row 20 to 50 cross into the tiles
    on the left, on the right and below, as does the ground."""
    f = np.full((CAP_H, CAP_W), DARK, np.uint8)
    f[1:1 + stripe_rows, 65:65 + stripe_cols:2] = LIGHT
    f[1 + stripe_rows, 65:65 + part:2] = LIGHT
    for r in range(comb_rows):
        if r % 2 == 0:
            f[1 + r, 65:65 + comb_cols:2] = LIGHT
        else:
            f[1 + r, 65:65 + comb_cols] = LIGHT
    if comb_part:
        f[1 + comb_rows, 65:65 + comb_part] = LIGHT
    for k in range(bars):
        f[24:26, 70 + 3 * k] = LIGHT
    for k in range(tweak):
        f[23 + 2 * k, 64] = LIGHT
    f[20, 40:151] = LIGHT
    f[20:51, 100] = LIGHT
    return salt(f)


@functools.lru_cache(maxsize=None)
def _capacity_search(what, target):
    """The first drawing whose tile under test has exactly `target` runs (what = "runs") or links ("links") and fewer than
    SEG_CAP of the other."""
    if what == "runs":
        for cols in range(62, 40, -1):
            for part in range(0, cols + 1):
                for tweak in (0, 1, 2):
                    f = _capacity_frame(cols, 7, part, 0, 0, 0, 0, tweak)
                    r, l = tile_counts(binary(f))[CAP_TILE]
                    if r == target and l < SEG_CAP:
                        return f
                    if r > target + 4:
                        break
                else:
                    continue
                break
    else:
        for cols in range(62, 30, -2):
            for part in range(0, cols + 1):
                for bars in (0, 1, 2):
                    f = _capacity_frame(0, 0, 0, 9, cols, part, bars, 0)
                    r, l = tile_counts(binary(f))[CAP_TILE]
                    if l == target and r < SEG_CAP:
                        return f
                    if l > target + 4:
                        break
                else:
                    continue
                break
    raise AssertionError("no drawing with %d %s" % (target, what))


CAPACITY_TARGETS = (("runs", 511), ("runs", 512), ("runs", 513), ("links", 512), ("links", 513))


def capacity():
    """192 x 64, one tile at the capacity of the common launch's tables: 511, 512, 513 runs with fewer links, and 512, 513
    links with fewer runs.  513 goes to k_seg_tile_dense, whose roots then merge with the common tiles' around it.
    Carries "counts" = (runs, links) of the tile under test and "dense" = tiles over the cap (0 or 1)."""
    cases = []
    for what, target in CAPACITY_TARGETS:
        f = _capacity_search(what, target).copy()
        cases.append(_case("capacity: %d %s" % (target, what), f, what=what, target=target, dense=1 if target > SEG_CAP else 0))
    return cases


def drawn():
    """every group-C frame outside the capacity cases"""
    return single_contacts() + last_column() + border_columns() + long_components() + seam_pairs() + label_batch()


def by_shape(cases):
    """[(f, [cases of one frame shape])], in the order of first appearance: what can share a device batch"""
    groups = {}
    for c in cases:
        groups.setdefault((c["f"], c["frame"].shape), []).append(c)
    return [(k[0], v) for k, v in groups.items()]
