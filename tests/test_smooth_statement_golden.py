"""The one NumPy statement of the sequence localisation (tests/smooth_ref.py, with tests/smooth_cov_ref.py; per-tag sizes
through tests/localize_ref.py) against what the statements it replaced (smooth_ref, its timed and rig copies, smooth_cov_ref)
returned at the last commit that had them, recorded in tests/golden/smooth_statements.npz by
tests/golden/make_smooth_statement_fixtures.py: the cases of the device comparisons and of the CPU statement tests, at their
huber_px and max_iters, plain and reversed.  The recorder's runs() is the list of calls and its compare() the comparison:
the numbers of frames, results, posed frames and trials and every integer field equal; every double -- the poses' T and rms,
the results' costs and rms, the covariances, the chain's d and tr and the cost of every trial -- byte for byte: measured on
the CPU with the recorder's compare, the largest difference over all 274 runs is 0, so the bound is 0.  No GPU."""
import functools
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "make_smooth_statement_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_smooth_statement_fixtures.py"))
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
    assert [r[0] for r in runs()] == list(record()) and {r[1] for r in runs()} == set(F.SETS) and len(runs()) == 274


@pytest.mark.parametrize("name", F.SETS)
def test_the_one_statement_returns_what_the_copies_returned(name):
    rec = record()
    worst = (0.0, "", "")
    for run in [r for r in runs() if r[1] == name]:
        worst = max(worst, F.compare(run[0], rec[run[0]], F.run_one(run)) + (run[0],))
    print("%s: largest relative difference %.3g" % (name, worst[0]))
    assert worst[0] <= BOUND, worst
