"""The NumPy statements of the solvers that take a tag map (tests/localize_ref.py with tests/rig_ref.py, tests/calib_ref.py,
tests/locate_ref.py), which state the per-tag size rule once, against what they and tests/sized_ref.py over them returned at
the last commit that had sized_ref.py, recorded in tests/golden/localize_statements.npz by
tests/golden/make_localize_statement_fixtures.py: the cases of the device comparisons and of the CPU statement tests, at their
gate, sigma_px, n_dist, flags and max_iters, and the sized cases through what were sized_ref's fronts.  The recorder's runs()
is the list of calls and its compare() the comparison: every integer field, seed_slot, every trace list, every T and every
covariance entry byte for byte; rms_px, rms_seed_px and the calibration result's K, dist, std and rms by their largest
relative difference: measured on the CPU with the recorder's compare, the largest over all 166 runs is 0 (the restated
functions were the originals' arithmetic in the same order, and moving them changed none of it), so the bound is 0.

With every size 0 this is what tests/test_sized_ref.py's test_no_sizes_is_localize_ref, test_no_sizes_is_rig_ref and
test_no_sizes_is_smooth_ref_and_calib_ref asserted of the patched statements: their calls are the runs camera/<exact,
mirrored, gate, slots, dist5>/s0.5, rig/back_to_back/s0.5 and calib/fronto/d0_i4 here, and the smooth call (smooth_cases.shape(5,
4, 0) at SHAPE_SIGMAS and COMPARE_ITERS) is plain/shape5_4_0/h0/fwd of tests/golden/smooth_statements.npz.  No GPU."""
import functools
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "make_localize_statement_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_localize_statement_fixtures.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

BOUND = 0.0


@functools.lru_cache(maxsize=None)
def record():
    return F.load()


@functools.lru_cache(maxsize=None)
def runs():
    return F.runs()


def test_every_recorded_run_is_compared_and_nothing_else():
    assert [r[0] for r in runs()] == list(record()) and {r[1] for r in runs()} == set(F.SETS) and len(runs()) == 166


def test_the_calls_of_the_retired_no_size_tests_are_recorded():
    keys = set(record())
    assert {"camera/%s/s0.5" % c for c in ("exact", "mirrored", "gate", "slots", "dist5")} <= keys
    assert {"rig/back_to_back/s0.5", "calib/fronto/d0_i4"} <= keys


@pytest.mark.parametrize("name", F.SETS)
def test_the_statements_return_what_they_returned_before_the_size_rule_moved(name):
    rec = record()
    worst = (0.0, "", "")
    for run in [r for r in runs() if r[1] == name]:
        worst = max(worst, F.compare(run[0], rec[run[0]], F.fields(run[2], F.run_one(run))) + (run[0],))
    print("%s: largest relative difference %.3g" % (name, worst[0]))
    assert worst[0] <= BOUND, worst
