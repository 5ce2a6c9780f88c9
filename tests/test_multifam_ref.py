"""The statement of a several-family detector (multifam_ref.py) on the mixed sheets of multifam_cases, without a GPU: it
finds exactly the placed tags, it equals the merged single-family oracle runs wherever the families are disjoint, and on
the alias pair it gives two detections per tag.  Then the CPU check of a family set, asl_families_check."""
import ctypes as C

import numpy as np
import pytest

import family_cases as FC
import multifam_cases as MC
import multifam_ref
from aprilslam_amd import _lib

MIXED = [MC.SETS["one_width"], MC.SETS["two_widths"], MC.SETS["min_width"], MC.SETS["four"], MC.ALL_SIX]


def same_detections(a, b):
    assert [d["id"] for d in a] == [d["id"] for d in b]
    for x, y in zip(a, b):
        assert x["hamming"] == y["hamming"] and np.float32(x["margin"]) == np.float32(y["margin"])
        assert np.array_equal(x["corners"], y["corners"]) and np.array_equal(x["center"], y["center"])


@pytest.mark.parametrize("turn", [0, 1])
@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("names", MIXED, ids="+".join)
def test_statement_finds_the_placed_tags_and_equals_the_single_family_runs(names, decimate, turn):
    fams, base = MC.families(names), MC.id_bases(names)
    img = MC.sheet(names, decimate, turn=turn)
    got = multifam_ref.detect(img, fams, base, decimate)
    want = MC.placed_ids(names, decimate)
    assert len(want) >= 6
    assert [d["id"] for d in got] == want and not any(d["hamming"] for d in got)
    same_detections(got, multifam_ref.merged_single_runs(img, fams, base, decimate))


@pytest.mark.parametrize("names", [MC.SETS["one_width"], MC.SETS["two_widths"], MC.SETS["four"]], ids="+".join)
def test_statement_on_the_shaded_and_the_damaged_sheet(names):
    fams, base = MC.families(names), MC.id_bases(names)
    want = MC.placed_ids(names, 1)
    got = MC.statement(names, 1, 0, shade=True)
    assert [d["id"] for d in got] == want
    same_detections(got, multifam_ref.merged_single_runs(MC.shaded(names, 1), fams, base, 1))
    got = MC.statement(names, 1, MC.DAMAGED)
    assert [d["id"] for d in got] == want and [d["hamming"] for d in got] == [1] * len(want)


@pytest.mark.parametrize("decimate", [1, 2])
def test_alias_pair_gives_two_detections_per_tag(decimate):
    """alias16 carries classic16's code (j + 5) % 24 under id j: tag k of the classic16 sheet is id k and id 24 + (k + 19) % 24"""
    names = MC.SETS["alias"]
    assert MC.id_bases(names) == (0, 24)
    n = FC.n_tags("classic16", decimate)
    got = MC.statement(names, decimate, 0)
    assert [d["id"] for d in got] == sorted(list(range(n)) + [24 + (k + 19) % 24 for k in range(n)])
    single = {d["id"]: d for d in FC.oracle_detections("classic16", decimate, 0)}
    for d in got:  # both detections of a tag are the quad the one-family oracle finds there
        k = d["id"] if d["id"] < 24 else (d["id"] - 24 + 5) % 24
        assert np.array_equal(d["corners"], single[k]["corners"]) and np.float32(d["margin"]) == np.float32(single[k]["margin"])


# ---- asl_families_check: a host function, no GPU

def _check(names, id_base=None, fams=None):
    _lib.families_check(list(fams if fams is not None else MC.families(names)), id_base)


def test_families_check_accepts_a_set_of_four():
    _check(MC.SETS["four"])
    _check(MC.SETS["four"], [1000, 0, 500, 65536 - 24])  # any order of the ranges, up to the last id 65535
    _check(("classic16",), [7])


def test_families_check_refuses_with_the_index_and_the_field():
    two = MC.SETS["two_widths"]
    with pytest.raises(_lib.AslError, match=r"n_fams must be in \[1, 4\] \(got 5\)"):
        _check(FC.NAMES[:5])
    with pytest.raises(_lib.AslError, match=r"n_fams must be in \[1, 4\] \(got 0\)"):
        _check(())
    bad = MC.family("circle21").to_dict()
    bad["width_at_border"] = 9
    from aprilslam_amd.families import TagFamily
    with pytest.raises(_lib.AslError, match=r"family 1: width_at_border"):
        _check(None, fams=[MC.family("classic25"), TagFamily.from_dict(bad)])
    with pytest.raises(_lib.AslError, match=r"family 1: id_base must not be negative \(got -1\)"):
        _check(two, [0, -1])
    with pytest.raises(_lib.AslError, match=r"family 1: id_base range \[23, 47\) overlaps that of family 0, \[0, 24\)"):
        _check(two, [0, 23])
    with pytest.raises(_lib.AslError, match=r"family 2: id_base range .* overlaps that of family 0"):
        _check(MC.SETS["one_width"], [100, 200, 90])
    with pytest.raises(_lib.AslError, match=r"family 1: id_base \+ ncodes must not exceed 65536"):
        _check(two, [0, 65536 - 23])
    _check(two, [24, 0])  # touching ranges do not overlap


def test_families_check_refuses_null_arrays():
    L = _lib.load()
    fs = _lib.FamilySet(MC.families(MC.SETS["two_widths"]))
    assert L.asl_families_check(None, fs.id_base_p, 2) == -1 and b"fams is NULL" in L.asl_last_error()
    assert L.asl_families_check(fs.c, None, 2) == -1 and b"id_base is NULL" in L.asl_last_error()
    assert L.asl_families_check(fs.c, fs.id_base_p, 2) == 0
    noarr = _lib.FamilySet(MC.families(MC.SETS["two_widths"]))
    noarr.c[1].codes = C.POINTER(C.c_uint64)()
    assert L.asl_families_check(noarr.c, noarr.id_base_p, 2) == -1 and b"family 1: codes is NULL" in L.asl_last_error()
