"""The ABI of the several-sequences call: include/aprilslam.h declares asl_smooth_sequences_device / _batch as the
single-sequence argument lists with `seq_start, n_seq` after the seed, the library exports them, and the ctypes argument lists
agree.  Then the conditions the GPU tests of tests/test_gpu_smooth_sequences.py rest on, evaluated with the statement
(tests/smooth_ref.py) on the batches of tests/smooth_seq_cases.py.  No GPU."""
import ctypes as C

import numpy as np

import smooth_cases as SC
import smooth_seq_cases as SQ
from aprilslam_amd import _lib
from test_smooth_cov_abi import prototype


def test_header_prototypes():
    cov, seq = prototype("asl_smooth_cov_frames_device"), prototype("asl_smooth_sequences_device")
    at = cov.index("d_seed") + 1
    assert seq == cov[:at] + ["seq_start", "n_seq"] + [{"d_result": "d_results"}.get(p, p) for p in cov[at:]]
    assert seq[-2:] == ["d_cov", "stream"] and "d_results" in seq and "d_result" not in seq
    cov, seq = prototype("asl_smooth_cov_batch"), prototype("asl_smooth_sequences_batch")
    at = cov.index("seed") + 1
    assert seq == cov[:at] + ["seq_start", "n_seq"] + [{"result": "results"}.get(p, p) for p in cov[at:]]


def test_exports_and_argtypes():
    L = _lib.load()
    for name in ("asl_smooth_sequences_device", "asl_smooth_sequences_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    extra = [C.POINTER(C.c_int32), C.c_int]
    dev, host = L.asl_smooth_cov_frames_device.argtypes, L.asl_smooth_cov_batch.argtypes
    assert L.asl_smooth_sequences_device.argtypes == dev[:11] + extra + dev[11:]
    assert L.asl_smooth_sequences_batch.argtypes == host[:11] + extra + host[11:]
    assert len(L.asl_smooth_sequences_device.argtypes) == len(prototype("asl_smooth_sequences_device")) == 21
    assert len(L.asl_smooth_sequences_batch.argtypes) == len(prototype("asl_smooth_sequences_batch")) == 20


def test_batches_are_what_the_issue_says():
    b = SQ.ragged(4)
    assert len(b.obs) == 270 and b.seq_start.tolist() == [0, 1, 3, 6, 11, 75, 140, 270] and b.obs.shape[1] == 4
    b1 = SQ.ragged(1)
    assert b1.obs.shape == (270, 1) and b1.seq_start.tolist() == b.seq_start.tolist()
    # mirrored seeds inside the one-tag batch: the statement's chain flips them back
    flipped = [SC.statement(n)[1]["n_flipped"] for n in SQ.ragged_names("1")]
    assert sum(flipped) > 0, flipped
    d = SQ.ragged_dist()
    assert d.seq_start.tolist() == [0, 5, 70] and len(d.dist) == 5
    m = SQ.many_short()
    assert len(m.seq_start) == 391 and len(m.obs) == 390 and np.all(np.diff(m.seq_start) == 1)
    assert m.obs[:130].tobytes() == m.obs[130:260].tobytes() == m.obs[260:].tobytes()
    p = SQ.short_pattern()
    assert len(p.obs) == 130 and np.diff(p.seq_start).tolist()[:5] == [1, 2, 3, 5, 1] and p.obs.tobytes() == m.obs[:130].tobytes()
    for batch in (b, b1, d, m, p, SQ.stop_apart(), SQ.failures()):
        assert batch.seq_start.dtype == np.int32 and batch.seq_start[0] == 0 and batch.seq_start[-1] == len(batch.obs) == len(batch.seed)
        assert np.all(np.diff(batch.seq_start) >= 1)


def test_failures_batch_statuses_by_the_statement():
    b = SQ.failures()
    assert np.diff(b.seq_start).tolist() == [7, 1, 6, 2, 7] and b.max_iters == 4
    runs = [SQ.statement(b, k) for k in range(5)]
    assert [int(r[1]["status"]) for r in runs] == SQ.FAILURES_STATUS == [0, 2, 1, 3, 0]
    assert runs[0][0]["status"].tolist() == [6, 0, 0, 6, 0, 0, 6]
    assert (runs[1][0]["status"] == 4).all() and (runs[3][0]["status"] == 4).all()
    assert (runs[2][0]["status"] == 1).all() and all(np.array_equal(T, np.eye(4)) for T in runs[2][0]["T"])
    assert [int(r[1]["iterations"]) for r in runs] == [runs[0][1]["iterations"], 4, 0, 0, runs[0][1]["iterations"]]


def test_stop_apart_batch_stops_apart_by_the_statement():
    b = SQ.stop_apart()
    assert SQ.ranges(b) == [(0, 40), (40, 41), (41, 43), (43, 56), (56, 82)] and b.max_iters == 30
    for k, c in enumerate(SQ.STOP_APART_CUTS):
        if c not in SQ.STOP_APART_TRIALS:
            continue
        a0, a1 = SQ.ranges(b)[k]
        for reverse in (False, True):
            res = SC.run(b.obs[a0:a1], b.rec, b.seed[a0:a1], None, b.sigmas, reverse=reverse, max_iters=b.max_iters)[1]
            assert res["status"] == 0 and res["iterations"] == SQ.STOP_APART_TRIALS[c] < b.max_iters, (c, reverse, res["iterations"])
    assert len(set(SQ.STOP_APART_TRIALS.values())) >= 2


def test_chunk_edge_cases_sit_on_the_kernels_chunk():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "aprilslam_amd", "csrc", "k_smooth.inc")).read()
    assert int(re.search(r"#define SM_SEQ_CHUNK (\d+)", src).group(1)) == SQ.SEQ_CHUNK
    for n in (SQ.SEQ_CHUNK, SQ.SEQ_CHUNK + 1, 910):
        b = SQ.past_one_chunk(n)
        assert len(b.seq_start) == n + 1 == len(b.obs) + 1 and b.obs[130:260].tobytes() == b.obs[:130].tobytes()
