"""The one NumPy statement of the tag-map reconstruction (tests/map_ref.py) against what the four statements it replaced
returned at the last commit that had them, recorded in tests/golden/map_statements.npz by
tests/golden/make_map_statement_fixtures.py: every case the device comparisons and the solver edge tests run, at their
huber_px and max_iters, plain and reversed.  The recorder's runs() is the list of calls and its compare() the comparison:
every integer field of the result and of the poses, valid, size and seed_slot equal; the map's T, the poses' T and slot_weight
byte for byte; cost, cost_seed, the result's and the frames' rms and tag_std within BOUND, relative.  No GPU."""
import functools
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "make_map_statement_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_map_statement_fixtures.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

# DEVICE_TOL's rule: ten times the largest relative difference the recorder's comparison measured over all 258 runs,
# 5.5e-16, at cost_seed of robust/behind/h0/i60/fwd: the single-camera statements summed the cost over all corners at once,
# the one statement sums it per view and then over the views.  A value above 1e-12 would mean more than a summation order.
MEASURED = 5.5e-16
BOUND = 10 * MEASURED


@functools.lru_cache(maxsize=None)
def record():
    return F.load()


@functools.lru_cache(maxsize=None)
def runs():
    return F.runs()


def test_every_recorded_run_is_compared_and_nothing_else():
    assert [r[0] for r in runs()] == list(record()) and {r[1] for r in runs()} == set(F.SETS) and len(runs()) == 258


@pytest.mark.parametrize("name", F.SETS)
def test_the_one_statement_returns_what_the_four_returned(name):
    rec = record()
    worst = (0.0, "", "")
    for run in [r for r in runs() if r[1] == name]:
        worst = max(worst, F.compare(run[0], rec[run[0]], F.run_one(run)) + (run[0],))
    print("%s: largest relative difference %.3g (%s of %s)" % ((name,) + worst))
    assert worst[0] <= BOUND, worst
