"""Six build-defined tag families that together walk every path of the decoder a family can choose, and the tag sheets
the family tests (CPU: test_family_tables.py, GPU: test_gpu_families.py) run on.

  name       nbits  wb  tw  border    why
  classic36  36     8   10  normal    64 border samples (one per lane), normal polarity
  classic25  25     7   9   normal    56 samples, centre bit
  classic16  16     6   8   normal    48 samples, 8 x 8 grid, 4-bit index chunks
  std52      52     6   10  reversed  more than 48 bits: whole-book search only
  circle21   21     5   9   reversed  40 samples (the shipped family's shape) with another layout
  custom48   48     6   10  reversed  48 bits: the widest indexed family, hole in the middle

Frames are 256 x 192 gray sheets (tag_sheet.py) with gap = 2 * cell + 4: cell 4 for decimate 1 (12 to 20 tags), cell 6 for
decimate 2 (6 tags).  A batch is five frames of one geometry: the sheet with every tag turned by 0, 90, 180 and 270
degrees in its place (the sheet is not square, so the tags turn, not the image), and the upright sheet with payload cell
(5k + 1) % nbits of tag k inverted.  Tag k carries id k.  `shaded` is the upright sheet once more, under a vignette: the
frame on which the fitted border sample set shows."""
import functools

import numpy as np

import tag_sheet
from aprilslam_amd import families

WIDTH, HEIGHT = 256, 192
NCODES = 24
CELL = {1: 4, 2: 6}  # decimate -> pixels per cell

_OUTER = [(x, -2) for x in range(-2, 7)]
# name: width_at_border, total_width, reversed_border, quadrant cells, centre, min_hamming.  min_hamming >= 5 wherever a
# test decodes at maxhamming 2 (classic36, std52); >= 3 everywhere, so that a word one bit off has one nearest code.
CASES = {
    "classic36": (8, 10, False, [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (2, 2), (3, 2), (4, 2), (3, 3)], None, 9),
    "classic25": (7, 9, False, [(1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (3, 2)], (3, 3), 6),
    "classic16": (6, 8, False, [(1, 1), (2, 1), (3, 1), (2, 2)], None, 3),
    "std52": (6, 10, True, _OUTER + [(1, 1), (2, 1), (3, 1), (2, 2)], None, 12),
    "circle21": (5, 9, True, [(1, -2), (2, -2), (3, -2), (1, 1), (2, 1)], (2, 2), 5),
    "custom48": (6, 10, True, _OUTER + [(1, 1), (2, 1), (3, 1)], None, 11),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def family(name):
    """The family, made once and registered under its name."""
    wb, tw, rev, quad, centre, mh = CASES[name]
    return families.register(families.make_family(name, wb, tw, rev, quad, centre=centre, ncodes=NCODES, min_hamming=mh, seed=7))


class _Drawn:
    """What tag_sheet draws: the family's tags turned by `turn` quarter turns, or with one payload cell inverted."""

    def __init__(self, fam, turn=0, damaged=False):
        self.fam, self.turn, self.damaged = fam, turn, damaged
        self.total_width = fam.total_width

    def grid(self, k):
        fam = self.fam
        g = fam.grid(k)
        if self.damaged:
            off = (fam.total_width - fam.width_at_border) // 2
            i = damaged_bit(fam, k)
            g[fam.bit_y[i] + off, fam.bit_x[i] + off] ^= 1
        return np.rot90(g, self.turn)


def damaged_bit(fam, k):
    return (5 * k + 1) % fam.nbits


def n_tags(name, decimate):
    fam, cell = family(name), CELL[decimate]
    return tag_sheet.capacity(fam, WIDTH, HEIGHT, cell, 2 * cell + 4)


def sheet(name, decimate, turn=0, damaged=False):
    fam, cell = family(name), CELL[decimate]
    return tag_sheet.tag_sheet(_Drawn(fam, turn, damaged), WIDTH, HEIGHT, cell, 2 * cell + 4, ids=lambda k: k)


DAMAGED = 4  # the batch's frame with the inverted cells


@functools.lru_cache(maxsize=None)
def batch(name, decimate):
    """(5, HEIGHT, WIDTH) uint8, read-only: turns 0..3, then the damaged sheet.  Every frame holds ids 0..n_tags-1."""
    frames = np.stack([sheet(name, decimate, turn=t) for t in range(4)] + [sheet(name, decimate, damaged=True)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def shaded(name, decimate):
    """(HEIGHT, WIDTH) uint8, read-only: the upright sheet with black at 40 under a vignette, 1 at the image's centre
    falling to 0.4 in its corners.  On the flat sheets every border sample of a colour reads the same value, and a plane
    fitted to a constant is that constant whichever samples are fitted: a decoder that leaves border samples out passes
    every frame of `batch` (tried: gray models cut at the 40th sample, all of test_gpu_families.py passed).  Under the
    vignette the white and the black border are curved surfaces, their fitted planes depend on the sample set, and the
    margin, compared as float32, pins it."""
    flat = sheet(name, decimate)
    y, x = np.mgrid[0:HEIGHT, 0:WIDTH]
    r2 = ((x + 0.5 - WIDTH / 2) / (WIDTH / 2)) ** 2 + ((y + 0.5 - HEIGHT / 2) / (HEIGHT / 2)) ** 2
    img = np.rint(np.where(flat > 0, 255.0, 40.0) * (1.0 - 0.3 * r2)).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def oracle_detections(name, decimate, frame, maxhamming=1):
    """The oracle's detections on one frame of the batch, computed once per session and shared."""
    import oracle_lib as O
    return tuple(O.detect_gray(batch(name, decimate)[frame], family(name), decimate, maxhamming=maxhamming))
