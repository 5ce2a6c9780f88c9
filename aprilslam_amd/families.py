"""Tag family tables for the AprilTag detector (host side).

The reference selects the family by name, `apriltag(tag_type)` with
tag_type="tagStandard41h12" (reference src/detection/tag_detector.py:17-18).  One code
table ships as data (aprilslam_amd/data/tagStandard41h12.json, written by
tools/gen_family.py): ids 0..4 are pinned by the reference's assets/tags/tag{0..4}.png,
ids >= 5 are build-defined.

Every other family is the user's to bring: a family is data (`TagFamily`), read from a dict,
a JSON file or the user's own copy of upstream's generated `tagXXhYY.c`
(`from_upstream_source`), and made known under its name with `register` / `load`.  The
detector then takes the name, or the `TagFamily` itself (`_lib.Detector(family=...)`).
No table under one of upstream's names is shipped or generated here: it would mislabel
printed tags.
"""
import json
import os
import re

import numpy as np

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
BUILTIN = "tagStandard41h12"


def rotate90(w, nbits):
    """The code word of the same tag turned by a quarter (upstream's rotate90)."""
    p, l = nbits, 0
    if nbits % 4 == 1:
        p, l = nbits - 1, 1
    w = ((w >> l) << (p // 4 + l)) | (w >> (3 * p // 4 + l) << l) | (w & l)
    return w & ((1 << nbits) - 1)


class TagFamily:
    def __init__(self, d):
        self.name = str(d["name"])
        self.nbits = int(d["nbits"])
        self.h = int(d.get("h", 0))
        self.width_at_border = int(d["width_at_border"])
        self.total_width = int(d["total_width"])
        self.reversed_border = bool(d["reversed_border"])
        self.bit_x = np.asarray(d["bit_x"], dtype=np.int32)
        self.bit_y = np.asarray(d["bit_y"], dtype=np.int32)
        self.codes = np.asarray([int(c, 16) if isinstance(c, str) else int(c) for c in d["codes"]], dtype=np.uint64)
        self.pinned_ids = int(d.get("pinned_ids", 0))
        if self.bit_x.shape != (self.nbits,) or self.bit_y.shape != (self.nbits,):
            raise ValueError("family %r: bit_x and bit_y must hold nbits = %d entries each" % (self.name, self.nbits))
        if self.codes.ndim != 1 or self.codes.shape[0] < 1:
            raise ValueError("family %r: codes must be a non-empty list" % (self.name,))

    @classmethod
    def from_dict(cls, d):
        """A family from its fields: name, nbits, width_at_border, total_width, reversed_border, bit_x, bit_y (upstream's
        convention: cell (0, 0) is the border's corner cell) and codes (hex strings or integers); h and pinned_ids optional."""
        return cls(d)

    @classmethod
    def from_json(cls, text):
        return cls(json.loads(text))

    def to_dict(self):
        return dict(name=self.name, nbits=self.nbits, h=self.h, width_at_border=self.width_at_border,
                    total_width=self.total_width, reversed_border=self.reversed_border,
                    bit_x=[int(v) for v in self.bit_x], bit_y=[int(v) for v in self.bit_y],
                    codes=["%x" % int(c) for c in self.codes], pinned_ids=self.pinned_ids)

    def to_json(self):
        return json.dumps(self.to_dict())

    @property
    def ncodes(self):
        return int(self.codes.shape[0])

    def grid(self, tag_id):
        """total_width x total_width uint8 cell grid (1 = white) of tag `tag_id`, as drawn upright."""
        tw, wb = self.total_width, self.width_at_border
        off = (tw - wb) // 2
        inner0, inner1 = off, off + wb - 1
        if self.reversed_border:
            # a white border ring on black: black just outside it and inside it, data overwrites
            g = np.zeros((tw, tw), dtype=np.uint8)
            g[inner0:inner1 + 1, inner0:inner1 + 1] = 1
            g[inner0 + 1:inner1, inner0 + 1:inner1] = 0
        else:
            # a black border square inside a white ring (everything outside the border), data overwrites the inside
            g = np.ones((tw, tw), dtype=np.uint8)
            g[inner0:inner1 + 1, inner0:inner1 + 1] = 0
        code = int(self.codes[tag_id])
        for i in range(self.nbits):
            bit = (code >> (self.nbits - 1 - i)) & 1
            g[self.bit_y[i] + off, self.bit_x[i] + off] = bit
        return g

    def texture(self, tag_id, cell_px=40):
        """RGB uint8 texture of the upright tag, `cell_px` texels per cell."""
        g = self.grid(tag_id)
        img = np.kron(g, np.ones((cell_px, cell_px), dtype=np.uint8)) * 255
        return np.repeat(img[:, :, None], 3, axis=2)


_CACHE = {}


def _shipped(name):
    return os.path.join(_DATA, name + ".json")


def is_registered(name):
    return name in _CACHE or os.path.exists(_shipped(name))


def get_family(name=BUILTIN):
    if name not in _CACHE:
        path = _shipped(name)
        if not os.path.exists(path):
            raise ValueError("unknown tag family: %r" % (name,))
        with open(path) as f:
            _CACHE[name] = TagFamily(json.load(f))
    return _CACHE[name]


def register(fam):
    """Make `fam` known under fam.name, so that get_family(name), apriltag(name), TagDetector(tag_type=name),
    SLAM(tag_type=name) and synth.render_frame(family=name) find it.  The built-in name stays the built-in table's: the
    detector reaches that one by name (with its five pinned ids), so give an own tagStandard41h12 table another name."""
    if not isinstance(fam, TagFamily):
        raise TypeError("register() takes a TagFamily")
    if fam.name == BUILTIN:
        raise ValueError("%r names the built-in table; register an own table under another name" % (BUILTIN,))
    _CACHE[fam.name] = fam
    return fam


def load(path):
    """Read a family from a JSON file (TagFamily.to_json's format) and register it."""
    with open(path) as f:
        return register(TagFamily.from_json(f.read()))


def _field(text, name, pattern=r"-?\d+"):
    m = re.search(r"(?:->|\.)\s*%s\s*=\s*(%s)\s*;" % (name, pattern), text)
    if not m:
        raise ValueError("upstream source: no assignment to `%s` found" % name)
    return m.group(1)


def from_upstream_source(text, name=None):
    """A TagFamily from the text of upstream's generated family source (`tagXXhYY.c`): the `codedata[N] = { 0x...UL, ... }`
    array and the assignments to nbits, h, width_at_border, total_width, reversed_border, bit_x[i] and bit_y[i] of its
    `..._create()` function, found by pattern wherever they stand.  This is how the real tables get here: whoever has
    upstream's detector has these files.  `name` defaults to the one in the text.  Raises ValueError naming what is missing."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    m = re.search(r"codedata\s*\[[^\]]*\]\s*=\s*\{([^}]*)\}", text)
    if not m:
        raise ValueError("upstream source: no complete `codedata[...] = { ... }` array found")
    codes = [int(c, 16) for c in re.findall(r"0[xX]([0-9a-fA-F]+)", m.group(1))]
    if not codes:
        raise ValueError("upstream source: the `codedata` array holds no codes")
    nbits = int(_field(text, "nbits"))
    d = dict(nbits=nbits, h=int(_field(text, "h")))  # in the order of upstream's file: a cut text names what it lacks first
    m = re.search(r"(?:->|\.)\s*ncodes\s*=\s*(\d+)\s*;", text)
    if m and int(m.group(1)) != len(codes):
        raise ValueError("upstream source: `ncodes` is %s but the `codedata` array holds %d codes" % (m.group(1), len(codes)))
    found = {axis: {int(i): int(v) for i, v in re.findall(r"(?:->|\.)\s*%s\s*\[\s*(\d+)\s*\]\s*=\s*(-?\d+)\s*;" % axis, text)}
             for axis in ("bit_x", "bit_y")}
    for i in range(nbits):
        for axis in ("bit_x", "bit_y"):
            if i not in found[axis]:
                raise ValueError("upstream source: no assignment to `%s[%d]` found" % (axis, i))
    d["bit_x"] = [found["bit_x"][i] for i in range(nbits)]
    d["bit_y"] = [found["bit_y"][i] for i in range(nbits)]
    d["width_at_border"] = int(_field(text, "width_at_border"))
    d["total_width"] = int(_field(text, "total_width"))
    d["reversed_border"] = _field(text, "reversed_border", r"true|false|0|1") in ("true", "1")
    if name is None:
        m = re.search(r"(?:->|\.)\s*name\s*=\s*(?:strdup\s*\(\s*)?\"([^\"]+)\"", text) or re.search(r"\b(tag\w+?)_create\s*\(", text)
        if not m:
            raise ValueError("upstream source: no family `name` found (pass name=...)")
        name = m.group(1)
    d["name"] = name
    d["codes"] = codes
    return TagFamily(d)


def make_family(name, width_at_border, total_width, reversed_border, quadrant_cells, centre=None, ncodes=24, min_hamming=3,
                seed=1):
    """A build-defined family for synthetic targets and tests: its codes are this function's, not any published table's,
    so it must never carry one of upstream's names nor be used to read printed tags of a published family.

    The layout comes from one quadrant's cells by the rotation rule the detector relies on: bits 0..q-1 are
    `quadrant_cells` (x, y) in order, bit i + q is bit i turned by a quarter, (width_at_border - 1 - y, x), and `centre`
    (if given) is the last bit.  The codes come from a seeded walk (a 64-bit linear congruential sequence, its top nbits)
    that keeps a word only if it is at least `min_hamming` from every rotation of every word kept so far and from its own
    three rotations."""
    wb, q = int(width_at_border), len(quadrant_cells)
    bx, by = [], []
    cells = [(int(x), int(y)) for x, y in quadrant_cells]
    for _ in range(4):
        bx += [c[0] for c in cells]
        by += [c[1] for c in cells]
        cells = [(wb - 1 - y, x) for x, y in cells]
    if centre is not None:
        bx.append(int(centre[0]))
        by.append(int(centre[1]))
    nbits = 4 * q + (1 if centre is not None else 0)
    if not 1 <= nbits <= 63:
        raise ValueError("make_family: nbits = %d is outside 1..63" % nbits)

    def dist(a, b):
        return bin(a ^ b).count("1")

    kept, rotations = [], []
    state = (int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
    for _ in range(200000):
        if len(kept) == ncodes:
            break
        state = (state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        w = state >> (64 - nbits)
        rots = [w]
        for _k in range(3):
            rots.append(rotate90(rots[-1], nbits))
        if min(dist(w, r) for r in rots[1:]) < min_hamming:
            continue
        if any(dist(w, r) < min_hamming for r in rotations):
            continue
        kept.append(w)
        rotations += rots
    if len(kept) < ncodes:
        raise ValueError("make_family: the walk found %d of %d codes at min_hamming %d" % (len(kept), ncodes, min_hamming))
    return TagFamily(dict(name=name, nbits=nbits, h=int(min_hamming), width_at_border=wb, total_width=int(total_width),
                          reversed_border=bool(reversed_border), bit_x=bx, bit_y=by, codes=kept))
