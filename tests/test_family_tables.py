"""Tag families as data, the host side: layouts and codes of make_family, the dict / JSON / upstream-source readers,
every refusal of asl_family_check (a pure host function: no GPU), and the condition the GPU family tests stand on --
the CPU oracle finds exactly the tags placed on every frame of every batch of family_cases."""
import numpy as np
import pytest

import family_cases as FC
import oracle_lib as O
from aprilslam_amd import _lib, families
from aprilslam_amd.families import TagFamily, get_family, rotate90


def with_code(fam, code):
    d = fam.to_dict()
    d["codes"] = [int(code)]
    return TagFamily.from_dict(d)


@pytest.mark.parametrize("name", FC.NAMES)
def test_layout_turns_with_the_code(name):
    fam = FC.family(name)
    wb, tw, rev, quad, centre, mh = FC.CASES[name]
    assert fam.nbits == 4 * len(quad) + (centre is not None) and fam.ncodes == FC.NCODES
    assert (fam.width_at_border, fam.total_width, fam.reversed_border) == (wb, tw, rev)
    cells = list(zip(fam.bit_x.tolist(), fam.bit_y.tolist()))
    assert len(set(cells)) == fam.nbits
    # the word of the tag turned by a quarter draws the grid turned by a quarter (counter-clockwise as an image)
    for code in fam.codes[:4]:
        assert np.array_equal(with_code(fam, rotate90(int(code), fam.nbits)).grid(0), np.rot90(with_code(fam, code).grid(0), 1))
    # the codes keep their distance over all rotations, a code's own included
    words = []
    for code in fam.codes:
        r = [int(code)]
        for _ in range(3):
            r.append(rotate90(r[-1], fam.nbits))
        assert min(bin(r[0] ^ x).count("1") for x in r[1:]) >= mh
        assert all(bin(r[0] ^ x).count("1") >= mh for x in words)
        words += r
    assert get_family(name) is fam  # registered under its name


def test_make_family_is_seeded():
    wb, tw, rev, quad, centre, mh = FC.CASES["circle21"]
    a = families.make_family("a", wb, tw, rev, quad, centre=centre, ncodes=8, min_hamming=mh, seed=3)
    b = families.make_family("b", wb, tw, rev, quad, centre=centre, ncodes=8, min_hamming=mh, seed=3)
    c = families.make_family("c", wb, tw, rev, quad, centre=centre, ncodes=8, min_hamming=mh, seed=4)
    assert np.array_equal(a.codes, b.codes) and not np.array_equal(a.codes, c.codes)
    with pytest.raises(ValueError, match="min_hamming"):
        families.make_family("d", 6, 8, False, FC.CASES["classic16"][3], ncodes=24, min_hamming=9)


def test_normal_border_grid_has_a_white_ring_outside_the_black_border():
    g = FC.family("classic36").grid(0)
    assert g[0].all() and g[-1].all() and g[:, 0].all() and g[:, -1].all()
    assert not g[1, 1:-1].any() and not g[-2, 1:-1].any() and not g[1:-1, 1].any() and not g[1:-1, -2].any()
    g = FC.family("std52").grid(0)  # reversed: a white border ring, black rings on both sides of it
    assert g[2, 2:-2].all() and g[-3, 2:-2].all() and g[2:-2, 2].all() and g[2:-2, -3].all()
    assert not g[1, 1:-1].any() and not g[-2, 1:-1].any() and not g[1:-1, 1].any() and not g[1:-1, -2].any()


def same_family(a, b):
    return (a.name, a.nbits, a.h, a.width_at_border, a.total_width, a.reversed_border) == \
        (b.name, b.nbits, b.h, b.width_at_border, b.total_width, b.reversed_border) and \
        np.array_equal(a.bit_x, b.bit_x) and np.array_equal(a.bit_y, b.bit_y) and np.array_equal(a.codes, b.codes)


@pytest.mark.parametrize("name", FC.NAMES + ("tagStandard41h12",))
def test_dict_and_json_round_trips(name, tmp_path):
    fam = get_family(name) if name.startswith("tag") else FC.family(name)
    assert same_family(TagFamily.from_dict(fam.to_dict()), fam)
    assert same_family(TagFamily.from_json(fam.to_json()), fam)
    if not name.startswith("tag"):
        d = fam.to_dict()
        d["name"] = name + "_from_file"
        p = tmp_path / "fam.json"
        p.write_text(TagFamily.from_dict(d).to_json())
        loaded = families.load(str(p))
        assert get_family(name + "_from_file") is loaded and np.array_equal(loaded.codes, fam.codes)


def test_the_builtin_name_cannot_be_shadowed():
    d = get_family().to_dict()
    with pytest.raises(ValueError, match="built-in"):
        families.register(TagFamily.from_dict(d))


def upstream_text(fam):
    """The family written the way upstream's generator writes a tagXXhYY.c"""
    n = fam.name
    lines = ['#include <stdlib.h>', '#include "%s.h"' % n, "",
             "static uint64_t codedata[%d] = {" % fam.ncodes]
    lines += ["   0x%016xUL," % int(c) for c in fam.codes]
    lines += ["};", "apriltag_family_t *%s_create()" % n, "{",
              "   apriltag_family_t *tf = calloc(1, sizeof(apriltag_family_t));",
              '   tf->name = strdup("%s");' % n, "   tf->h = %d;" % fam.h, "   tf->ncodes = %d;" % fam.ncodes,
              "   tf->codes = codedata;", "   tf->nbits = %d;" % fam.nbits,
              "   tf->bit_x = calloc(%d, sizeof(uint32_t));" % fam.nbits, "   tf->bit_y = calloc(%d, sizeof(uint32_t));" % fam.nbits]
    for i in range(fam.nbits):
        lines += ["   tf->bit_x[%d] = %d;" % (i, fam.bit_x[i]), "   tf->bit_y[%d] = %d;" % (i, fam.bit_y[i])]
    lines += ["   tf->width_at_border = %d;" % fam.width_at_border, "   tf->total_width = %d;" % fam.total_width,
              "   tf->reversed_border = %s;" % ("true" if fam.reversed_border else "false"), "   return tf;", "}", ""]
    return "\n".join(lines)


@pytest.mark.parametrize("name", ["classic36", "std52", "circle21"])
def test_from_upstream_source_reads_the_family_back(name, tmp_path):
    fam = FC.family(name)
    p = tmp_path / (name + ".c")
    p.write_text(upstream_text(fam))
    back = families.from_upstream_source(p.read_text())
    assert same_family(back, fam)
    assert families.from_upstream_source(p.read_text(), name="mine").name == "mine"
    _lib.family_check(back)


def test_from_upstream_source_names_what_a_truncated_text_lacks():
    fam = FC.family("classic25")
    text = upstream_text(fam)
    with pytest.raises(ValueError, match="codedata"):
        families.from_upstream_source(text[:text.index("};") - 40])  # cut inside the code array
    with pytest.raises(ValueError, match=r"bit_y\[17\]"):
        families.from_upstream_source(text[:text.index("tf->bit_y[17]")])
    with pytest.raises(ValueError, match="width_at_border"):
        families.from_upstream_source(text[:text.index("tf->width_at_border")])
    with pytest.raises(ValueError, match="reversed_border"):
        families.from_upstream_source(text[:text.index("tf->reversed_border")])
    with pytest.raises(ValueError, match="ncodes"):
        families.from_upstream_source(text.replace("   0x%016xUL,\n" % int(fam.codes[3]), ""))


# ---- asl_family_check

@pytest.mark.parametrize("name", FC.NAMES + ("tagStandard41h12",))
def test_family_check_passes_the_families_in_use(name):
    _lib.family_check(get_family(name) if name.startswith("tag") else FC.family(name))


def changed(name, **kw):
    """The family's dict with fields replaced; bit_x / bit_y / codes also as {index: value}"""
    d = FC.family(name).to_dict()
    d["codes"] = [int(c, 16) for c in d["codes"]]
    for k, v in kw.items():
        if isinstance(v, dict):
            for i, x in v.items():
                d[k][i] = x
        else:
            d[k] = v
    return d


REFUSALS = [
    # (what, family dict, the message names)
    ("nbits 0", changed("classic16", nbits=0), r"nbits must be in \[1, 63\]"),
    ("nbits 64", changed("classic16", nbits=64), r"nbits must be in \[1, 63\]"),
    ("nbits % 4 == 2", changed("classic16", nbits=18), r"nbits % 4 must be 0 or 1"),
    ("nbits % 4 == 3", changed("classic16", nbits=15), r"nbits % 4 must be 0 or 1"),
    ("border of 1", changed("classic16", width_at_border=1), r"width_at_border must be in \[2, 8\]"),
    ("border of 9", changed("classic16", width_at_border=9), r"width_at_border must be in \[2, 8\]"),
    ("grid of 18", changed("classic16", total_width=18), "total_width"),
    ("grid below the border", changed("classic16", total_width=4), "total_width"),
    ("odd difference", changed("classic16", total_width=9), "total_width"),
    ("no codes", changed("classic16", codes=[]), r"ncodes must be in \[1, 65535\]"),
    ("65536 codes", changed("classic16", codes=list(range(65536))), r"ncodes must be in \[1, 65535\]"),
    ("code too wide", changed("classic16", codes={5: 1 << 16}), r"codes\[5\] has bits at or above nbits"),
    ("duplicate code", changed("classic16", codes={9: int(FC.family("classic16").codes[2])}), r"codes\[9\] is a duplicate of codes\[2\]"),
    ("cell outside the grid", changed("circle21", bit_x={0: 7}), r"bit 0 at \(7, -2\) is outside the total_width grid"),
    ("two bits on a cell", changed("classic36", bit_x={1: 1}), r"bit 0 and bit 1 share the cell \(1, 1\)"),
    ("cell on the border ring", changed("classic36", bit_y={2: 0}), r"bit 2 at \(3, 0\) is on the border ring"),
    ("cell on the far border ring", changed("std52", bit_x={9: 5}), r"bit 9 at \(5, 1\) is on the border ring"),
    ("cell on the ring outside", changed("std52", bit_y={3: -1}), r"bit 3 at \(1, -1\) is on the ring just outside the border"),
    ("cell on the far ring outside", changed("custom48", bit_x={4: 6}, bit_y={4: 3}), r"bit 4 at \(6, 3\) is on the ring just outside"),
    # moved to cells that are free, so that only the rotation rule objects
    ("layout does not turn", changed("custom48", bit_x={21: 2}, bit_y={21: 2}), r"does not turn with the code: bit 21 must be at \(4, 1\)"),
    ("last bit off the centre", changed("circle21", bit_x={20: 0}, bit_y={20: -2}), "last bit must be at the centre"),
]


class _Raw:
    """A family as asl_family_check gets it, without TagFamily's own checks"""

    def __init__(self, d):
        self.__dict__.update(d)


@pytest.mark.parametrize("what,d,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_family_check_refuses(what, d, message):
    with pytest.raises(_lib.AslError, match=message):
        _lib.family_check(_Raw(d))


def test_family_check_refuses_null_arrays():
    import ctypes as C
    L = _lib.load()
    for field in ("bit_x", "bit_y", "codes"):
        t = _lib.FamilyTable(FC.family("classic16"))
        setattr(t.c, field, C.POINTER(C.c_uint64 if field == "codes" else C.c_int32)())
        assert L.asl_family_check(C.byref(t.c)) == -1
        assert (field + " is NULL").encode() in L.asl_last_error()
    assert L.asl_family_check(None) == -1 and b"family is NULL" in L.asl_last_error()


# ---- the oracle on the sheets: what the GPU tests compare with

@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_finds_exactly_the_tags_placed(name, decimate):
    fam = FC.family(name)
    n = FC.n_tags(name, decimate)
    assert (12 <= n <= 20) if decimate == 1 else n == 6
    for f in range(5):
        dets = FC.oracle_detections(name, decimate, f)
        assert [r["id"] for r in dets] == list(range(n)), (name, decimate, f)
        assert [r["hamming"] for r in dets] == [1 if f == FC.DAMAGED else 0] * n
    assert O.detect_gray(FC.batch(name, decimate)[FC.DAMAGED], fam, decimate, maxhamming=0) == []


@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("name", FC.NAMES)
def test_oracle_finds_the_tags_on_the_shaded_sheet(name, decimate):
    dets = O.detect_gray(FC.shaded(name, decimate), FC.family(name), decimate)
    assert [r["id"] for r in dets] == list(range(FC.n_tags(name, decimate)))
    assert not any(r["hamming"] for r in dets)
