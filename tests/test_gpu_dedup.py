"""The device de-duplication stage (S8, csrc/k_dedup.inc) at its group, size and capacity edges.

asl_debug_dedup runs the stage's four kernels on records of the test's own, through the launches a batch uses, and is held
to the plain statement tests/dedup_ref.py byte for byte: survivors, their order, the per-frame counts and the counters
(tests/test_dedup_ref.py holds the statement to the C oracle on the same cases, on the CPU).  The tag-sheet tests then
push frames of 256 to 1025 tags through the whole detector: the host's growth of the per-frame lists, the refusal above
1024 detections in a frame, and the staging of the read-back.  Bars of tests/stage_check.py: ids, hamming, margin and
order exact, corners within CORNER_TOL."""
import time

import numpy as np
import pytest

import dedup_cases as DC
import dedup_ref as R
import oracle_lib as O
import tag_sheet as TS
from aprilslam_amd import _lib, synth
from stage_check import CORNER_TOL

pytestmark = pytest.mark.gpu

CASES = DC.all_cases()


@pytest.fixture(scope="module")
def det():
    d = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    yield d
    d.close()


def assert_equals_statement(det, case):
    out, npf, cnt = det.debug_dedup(case.recs, case.keys, case.n_frames, case.cap)
    want, want_npf, want_cnt = R.dedup(case.recs, case.keys, case.n_frames, case.cap)
    assert npf.tolist() == want_npf.tolist(), case.name
    if want_cnt[1]:  # how many records find the list full before the launch backs out is not defined
        assert cnt[1] > 0 and cnt[0] == 0 and cnt[2] == want_cnt[2], (case.name, cnt)
    else:
        assert cnt.tolist() == want_cnt.tolist(), (case.name, cnt, want_cnt)
    if out.tobytes() != want.tobytes():
        bad = [i for i in range(min(len(out), len(want))) if out[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: %d records for %d, first difference at %s: %s / %s" % (
            case.name, len(out), len(want), bad[:1], out[bad[:1]], want[bad[:1]]))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stage_equals_the_statement(det, case):
    t0 = time.perf_counter()
    assert_equals_statement(det, case)
    if case.name.startswith("one_id"):  # the single-lane worst cases: DESIGN.md quotes the time, nothing asserts on it
        print("%s: %.3f s for the call" % (case.name, time.perf_counter() - t0))


def test_hand_frames_one_by_one(det):
    """every hand and chain frame as a call of its own, so that a failure names the frame"""
    case, labels = DC.hand_case()
    for f, label in enumerate(labels):
        m = case.recs["frame"] == f
        r = case.recs[m].copy()
        r["frame"] = 0
        assert_equals_statement(det, DC.Case(label, r, case.keys[m], 1, case.cap))


def test_memory_order_does_not_matter(det):
    """the same records permuted in memory, each keeping its key: identical output bytes"""
    rng = np.random.default_rng(99)
    for case in (DC.size_case(513, "mix"), DC.placement_case(), DC.frames_case(65)):
        first = det.debug_dedup(case.recs, case.keys, case.n_frames, case.cap)
        for _ in range(3):
            p = rng.permutation(len(case.recs))
            again = det.debug_dedup(case.recs[p], case.keys[p], case.n_frames, case.cap)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), case.name


def test_the_hook_refuses_what_it_cannot_run_and_touches_nothing(det, family):
    """asl_debug_dedup through ctypes as the binding calls it: every refusal is ASL_EINVAL with the need in the message and
    leaves the sentinel-filled outputs alone; a run leaves the detector's last batch as it was."""
    import torch
    img = TS.tag_sheet(family, 640, 360, 4, 12, n=5)
    dets0, npf0 = det.detect_host(img, channels=1)
    assert len(dets0) == 5
    counters0 = det.debug_counters().copy()
    case = DC.frames_case(2)
    n = len(case.recs)
    recs, keys = np.ascontiguousarray(case.recs), np.ascontiguousarray(case.keys)
    out = np.full(n * _lib.DET_DTYPE.itemsize, 0xA5, dtype=np.uint8)
    npf = np.full(2, -7, dtype=np.int32)
    cnt = np.full(3, -7, dtype=np.int64)
    L, h = det._L, det._h

    def call(recs=recs.ctypes.data, keys=keys.ctypes.data, n=n, n_frames=2, cap=4, out=out.ctypes.data, max_out=n, npf=npf.ctypes.data,
             cnt=cnt.ctypes.data, n_cnt=3, handle=h):
        return L.asl_debug_dedup(handle, recs, keys, n, n_frames, cap, out, max_out, npf, cnt, n_cnt)

    def refused(rc, need):
        assert rc == -1, rc  # ASL_EINVAL
        msg = L.asl_last_error().decode()
        assert need in msg, msg
        assert (out == 0xA5).all() and (npf == -7).all() and (cnt == -7).all()

    for name in ("handle", "recs", "keys", "out", "npf", "cnt"):
        refused(call(**{name: None}), "NULL argument")
    refused(call(n_frames=0), "n_frames must be in [1, 65535]")
    refused(call(n_frames=-3), "n_frames must be in [1, 65535]")
    refused(call(cap=0), "cap_per_frame must be >= 1")
    refused(call(n=-1), "n must be >= 0")
    for frame in (-1, 2):
        bad = recs.copy()
        bad["frame"][n - 1] = frame
        refused(call(recs=bad.ctypes.data), "record %d: frame %d is outside [0, 2)" % (n - 1, frame))
    refused(call(max_out=n - 1), "need %d records" % n)
    refused(call(n_cnt=2), "need 3 values")
    t = torch.from_numpy(img).to("cuda:0")
    det.submit_device(t.data_ptr(), 1, 1, img.shape[1], img.shape[0])
    try:
        refused(call(), "a batch is in flight")
    finally:
        det.collect()

    assert call() == 0  # exactly enough room is enough
    want, want_npf, want_cnt = R.dedup(case.recs, case.keys, 2, 4)
    assert npf.tolist() == want_npf.tolist() and cnt.tolist() == want_cnt.tolist()
    assert out[:len(want) * 96].tobytes() == want.tobytes() and (out[len(want) * 96:] == 0xA5).all()
    assert (det.debug_counters() == counters0).all()
    dets1, npf1 = det.detect_host(img, channels=1)
    assert dets1.tobytes() == dets0.tobytes() and npf1.tolist() == npf0.tolist()


# ---- end to end on tag sheets

SHEET = (1280, 720, 4, 12)      # 364 places, decimate 1
BIG_SHEET = (1600, 1584, 4, 12)  # 1056 places
HALF_SHEET = (1920, 1080, 6, 18)  # 364 places, decimate 2


def assert_equals_oracle(mine, gray, family, decimate):
    ref = O.detect_gray(gray, family, decimate, cap=2048)
    assert [int(d["id"]) for d in mine] == [r["id"] for r in ref]
    for d, r in zip(mine, ref):
        assert int(d["hamming"]) == r["hamming"]
        assert np.float32(d["margin"]) == np.float32(r["margin"])
        assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL and np.abs(d["center"] - r["center"]).max() <= CORNER_TOL
    return ref


@pytest.mark.parametrize("n", [256, 257, 1024])
def test_a_frame_at_the_edges_of_the_list_capacity(family, n):
    """256 tags fill the initial per-frame list exactly, 257 overflow it (the host grows it fourfold and runs the batch again),
    1024 fill what the sort holds.  The 256-tag frame goes through detect_device with its default room of 64 records, so the
    binding's own second call runs too."""
    import torch
    img = TS.tag_sheet(family, *(SHEET if n <= 364 else BIG_SHEET), n=n)
    det = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    try:
        if n == 256:
            t = torch.from_numpy(img).to("cuda:0")
            dets, _, npf = det.detect_device(t.data_ptr(), 1, 1, img.shape[1], img.shape[0])
        else:
            dets, npf = det.detect_host(img, channels=1, max_per_frame=n)
        assert npf.tolist() == [n] and len(dets) == n
        assert_equals_oracle(dets, img, family, 1)
        c = det.debug_counters()  # [6] detections decoded, [10] the list capacity (one frame), [14] records past a full list
        assert c[6] >= n and c[14] == 0 and c[10] == (256 if c[6] <= 256 else 1024), c
        assert n != 257 or c[10] == 1024
    finally:
        det.close()


def test_a_frame_above_the_sort_capacity_fails_loudly(family):
    det = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    try:
        with pytest.raises(_lib.AslError) as e:
            det.detect_host(TS.tag_sheet(family, *BIG_SHEET, n=1025), channels=1, max_per_frame=1100)
        assert "de-duplication" in str(e.value) and "more than 1024 detections" in str(e.value), str(e.value)
        img = TS.tag_sheet(family, *SHEET, n=256)
        dets, npf = det.detect_host(img, channels=1)
        assert npf.tolist() == [256]
        assert_equals_oracle(dets, img, family, 1)
    finally:
        det.close()


@pytest.mark.parametrize("sheet,decimate", [(SHEET, 1), (HALF_SHEET, 2)], ids=["decimate1", "decimate2"])
def test_sheets_of_repeated_ids(family, sheet, decimate):
    """364 tags of seven ids: groups of 52 of one id in every frame, none of which overlap"""
    img = TS.tag_sheet(family, *sheet, ids=lambda k: k % 7)
    det = _lib.Detector("tagStandard41h12", decimate=float(decimate), id_limit=0)
    try:
        dets, npf = det.detect_host(img, channels=1, max_per_frame=400)
        assert npf.tolist() == [364]
        assert_equals_oracle(dets, img, family, decimate)
    finally:
        det.close()


def test_read_back_staging_across_batches_of_very_different_size(family):
    """One detector, batches of 40, 728, 4368, 40 and 728 detections with poses: the first has no prefetch; the second grows the
    lists and runs again; the third prefetches the second's guess, finds more results than the page-locked staging (4096
    records) holds and replaces it; the fourth is covered by its prefetch; the fifth prefetches the fourth's guess (306 records)
    and fetches the rest with the partial second copy.  Every frame equals the oracle, every batch a fresh detector's bytes,
    and every pose the device PnP of the corners beside it."""
    K = synth.camera_matrix(SHEET[0], SHEET[1])
    dist, tag_size = np.zeros(4), 10.0

    def frame(n, f):
        return TS.tag_sheet(family, *SHEET, n=n, ids=lambda k: (k + 31 * f) % 512)

    small = np.stack([frame(20, f) for f in range(2)])
    large = np.stack([frame(364, f) for f in range(12)])
    refs = {}

    def run(det, frames):
        return det.detect_host(frames, channels=1, max_per_frame=400, K=K, dist=dist, tag_size=tag_size)

    det = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    try:
        for name, frames in (("small", small), ("two", large[:2]), ("twelve", large), ("small", small), ("two", large[:2])):
            dets, poses, npf = run(det, frames)
            assert npf.tolist() == [20 if name == "small" else 364] * len(frames) and len(dets) == len(poses) == npf.sum()
            assert np.array_equal(dets["frame"], np.repeat(np.arange(len(frames)), npf))
            if name not in refs:
                fresh = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
                try:
                    refs[name] = run(fresh, frames)
                finally:
                    fresh.close()
                start = 0
                for b in range(len(frames)):
                    assert_equals_oracle(refs[name][0][start:start + npf[b]], frames[b], family, 1)
                    start += npf[b]
            assert all(a.tobytes() == b.tobytes() for a, b in zip((dets, poses, npf), refs[name])), name
            rvec, tvec, T, ok = det.solve_pnp(dets["corners"], K, dist, tag_size)
            assert np.array_equal(poses["ok"].astype(bool), ok)
            assert poses["rvec"].tobytes() == rvec.tobytes() and poses["tvec"].tobytes() == tvec.tobytes()
            assert poses["T"].tobytes() == T.tobytes()
    finally:
        det.close()
