"""The sequence localisation with frame times on the device (asl_smooth_timed_sequences_device / _batch: SmoothBufs.times in
k_smooth.inc) against the NumPy statement (tests/smooth_ref.py) on the cases and recorded figures of
tests/smooth_timed_cases.py, and without times or at unit spacing against the existing entry points, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_ref as SR
import smooth_seq_cases as SQ
import smooth_timed_cases as TC
import solver_checks as CK
from aprilslam_amd import _lib, synth
from aprilslam_amd._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in TC.all_cases()}
PLAIN = {c[0]: c[1:] for c in SC.all_cases()}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
HUBER = 0.6     # the positive threshold of the comparisons with the robust entry point (smooth_robust_cases' own)


def _camera(dist):
    Kc = np.ascontiguousarray(SC.K, dtype=np.float64)
    dc = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64)
    return Kc, dc, (Kc.ctypes.data_as(DP), None if dc is None else dc.ctypes.data_as(DP), 0 if dc is None else len(dc), SC.TAG)


def entry(form, huber, timed):
    """(function, the arguments between sigma_trans and max_iters): timed -> asl_smooth_timed_sequences_*, else huber None ->
    asl_smooth_sequences_*, else asl_smooth_robust_sequences_*"""
    L = _lib.load()
    name = "timed" if timed else "plain" if huber is None else "robust"
    fn = {"timed": "asl_smooth_timed_sequences_", "robust": "asl_smooth_robust_sequences_", "plain": "asl_smooth_sequences_"}[name] + form
    return getattr(L, fn), (() if name == "plain" else (float(huber or 0.0),))


def host(det, obs, start, rec, dist, sigmas, huber, iters, seed, times=None, with_cov=True, timed=True):
    """the host form through ctypes -> (rc, poses, results, cov or None); timed False: the entry point without the argument"""
    o, sd, st = np.ascontiguousarray(obs), None if seed is None else np.ascontiguousarray(seed), np.ascontiguousarray(start, dtype=np.int32)
    tm = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    n, mt = o.shape
    Kc, dc, cam = _camera(dist)
    out, res = np.zeros(n, dtype=CAM_POSE_DTYPE), np.zeros(len(st) - 1, dtype=SMOOTH_RESULT_DTYPE)
    cov = np.zeros(n, dtype=POSE_COV_DTYPE) if with_cov else None
    fn, extra = entry("batch", huber, timed)
    targ = ((None if tm is None else tm.ctypes.data_as(DP)),) if timed else ()
    rc = fn(det._h, o.ctypes.data, n, mt, rec.ctypes.data, len(rec), *cam, None if sd is None else sd.ctypes.data, *targ, st.ctypes.data_as(IP),
            len(st) - 1, *sigmas, *extra, iters, out.ctypes.data, res.ctypes.data, None if cov is None else cov.ctypes.data)
    return rc, out, res, cov


class OnDevice:
    """a block on device buffers; run(): one enqueue on a stream of its own, then the outputs' bytes"""

    def __init__(self, det, obs, rec, seed):
        import torch
        self.torch, self.det, self.dev = torch, det, torch.device("cuda:0")
        self.n, self.mt, self.n_ids = obs.shape[0], obs.shape[1], len(rec)
        self.d_obs, self.d_map, self.d_seed = CK.dev_bytes(obs, self.dev), CK.dev_bytes(rec, self.dev), CK.dev_bytes(seed, self.dev)
        self.stream = torch.cuda.Stream(self.dev)

    def outputs(self, n_seq, fill=0):
        t = self.torch
        out = [t.full((size,), fill, dtype=t.uint8, device=self.dev)
               for size in (self.n * CAM_POSE_DTYPE.itemsize, n_seq * SMOOTH_RESULT_DTYPE.itemsize, self.n * POSE_COV_DTYPE.itemsize)]
        t.cuda.synchronize()
        return out

    def args(self, start, dist, sigmas, huber, iters, out, with_cov, times=None, timed=True):
        st = np.ascontiguousarray(start, dtype=np.int32)
        Kc, dc, cam = _camera(dist)
        d_times = None if times is None else CK.dev_bytes(np.ascontiguousarray(times, dtype=np.float64), self.dev)
        self.torch.cuda.synchronize()
        keep = (st, Kc, dc, d_times)
        fn, extra = entry("device", huber, timed)
        targ = ((None if d_times is None else d_times.data_ptr()),) if timed else ()
        return keep, fn, [self.det._h, self.d_obs.data_ptr(), self.n, self.mt, self.d_map.data_ptr(), self.n_ids, *cam, self.d_seed.data_ptr(), *targ,
                          st.ctypes.data_as(IP), len(st) - 1, *sigmas, *extra, iters, out[0].data_ptr(), out[1].data_ptr(),
                          out[2].data_ptr() if with_cov else None, self.stream.cuda_stream]

    def run(self, start, dist, sigmas, huber, iters, times=None, with_cov=True, timed=True):
        out = self.outputs(len(start) - 1)
        keep, fn, a = self.args(start, dist, sigmas, huber, iters, out, with_cov, times, timed)
        assert fn(*a) == 0, _lib.load().asl_last_error()
        self.stream.synchronize()
        return tuple(o.cpu().numpy().tobytes() for o in out)


_runs = {}


def device_case(det, name):
    """(poses, result, cov) of the host form with cov on a case of smooth_timed_cases.all_cases(), run once"""
    if name not in _runs:
        obs, rec, seed, dist, times, sig, iters = CASES[name]
        rc, out, res, cov = host(det, obs, [0, len(obs)], rec, dist, sig, 0.0, iters, seed, times)
        assert rc == 0
        _runs[name] = (out, res[0], cov)
    return _runs[name]


def close(a, b, rel=1e-6):
    return abs(a - b) <= rel * max(1.0, abs(b))


def assert_same(name, got, gres, want, wres):
    """every field of the device's records against the timed statement's"""
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d / %d, cost %.12g / %.12g" %
          (name, worst, TC.DEVICE_TOL, gres["iterations"], wres["iterations"], gres["cost"], wres["cost"]))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    for k in ("n_frames_data", "n_filled", "n_flipped", "status", "iterations", "n_soft"):
        assert gres[k] == wres[k], (name, k, gres[k], wres[k])
    assert not np.any(gres["reserved"]) and gres["n_soft"] == got["n_rejected"].sum()
    assert worst <= TC.DEVICE_TOL, (name, worst)
    for k in ("rms_px", "rms_seed_px"):
        assert all(close(g, w) for g, w in zip(got[k], want[k])), (name, k)
        assert close(gres[k], wres[k]), (name, k)
    for k in ("cost", "cost_seed"):
        assert close(gres[k], wres[k]), (name, k, gres[k], wres[k])


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_the_statement(gpu_detector, name):
    got, gres, _ = device_case(gpu_detector, name)
    want, wres, _ = TC.statement(name)
    assert_same(name, got, gres, want, wres)
    if name.startswith("shape") and len(got) > 1:     # the times took part: not the plain call's bytes
        obs, rec, seed, dist, times, sig, iters = CASES[name]
        rc, p0, r0, _ = host(gpu_detector, obs, [0, len(obs)], rec, dist, sig, 0.0, iters, seed, None)
        assert rc == 0 and p0.tobytes() != got.tobytes()


def unit_times(start):
    """5 + the frame's index in its sequence: unit spacing with exact differences, going back at every boundary"""
    return np.concatenate([5.0 + np.arange(b - a) for a, b in zip(start[:-1], start[1:])])


def assert_is_the_existing_call(det, obs, start, rec, seed, dist, sig, iters):
    dv = OnDevice(det, obs, rec, seed)
    unit = unit_times(start)
    for with_cov in (True, False):
        for huber in (0.0, HUBER):
            rc0, p0, r0, c0 = host(det, obs, start, rec, dist, sig, huber, iters, seed, with_cov=with_cov, timed=False)
            d0 = dv.run(start, dist, sig, huber, iters, with_cov=with_cov, timed=False)
            assert rc0 == 0 and d0[0] == p0.tobytes() and d0[1] == r0.tobytes()
            for times in (None, unit):
                rc1, p1, r1, c1 = host(det, obs, start, rec, dist, sig, huber, iters, seed, times, with_cov)
                assert rc1 == 0 and p0.tobytes() == p1.tobytes() and r0.tobytes() == r1.tobytes(), (with_cov, huber, times is None)
                assert (c0 is None and c1 is None) or c0.tobytes() == c1.tobytes(), (with_cov, huber, times is None)
                assert dv.run(start, dist, sig, huber, iters, times, with_cov) == d0, (with_cov, huber, times is None)
            if huber == 0.0:        # and through the robust call the plain one
                rc2, p2, r2, c2 = host(det, obs, start, rec, dist, sig, None, iters, seed, with_cov=with_cov, timed=False)
                assert rc2 == 0 and p0.tobytes() == p2.tobytes() and r0.tobytes() == r2.tobytes()
                assert (c0 is None and c2 is None) or c0.tobytes() == c2.tobytes()
                assert dv.run(start, dist, sig, None, iters, with_cov=with_cov, timed=False) == d0


@pytest.mark.parametrize("name", list(PLAIN))
def test_no_times_and_unit_times_are_the_existing_calls(gpu_detector, name):
    """d_times NULL and times = 5 + arange through the new entry points: the robust entry point's bytes at huber 0 and at a
    positive huber, host and device forms, with and without d_cov; through it the plain calls' bytes"""
    obs, rec, seed, dist, sig, iters = PLAIN[name]
    assert_is_the_existing_call(gpu_detector, obs, [0, len(obs)], rec, seed, dist, sig, iters)


def test_no_times_and_unit_times_are_the_existing_calls_on_a_batch(gpu_detector):
    b = SQ.failures()
    assert_is_the_existing_call(gpu_detector, b.obs, b.seq_start, b.rec, b.seed, b.dist, b.sigmas, b.max_iters)


@pytest.mark.parametrize("max_tags", [1, 4])
def test_each_sequence_of_a_batch_is_the_call_alone(gpu_detector, max_tags):
    b, times = TC.ragged(max_tags)
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed, times)
    assert rc == 0 and (results["status"] == 0).all() and (cov["status"] == 0).all()
    for k, (a0, a1) in enumerate(SQ.ranges(b)):
        rc1, p1, r1, c1 = host(gpu_detector, b.obs[a0:a1], [0, a1 - a0], b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed[a0:a1], times[a0:a1])
        assert rc1 == 0 and poses[a0:a1].tobytes() == p1.tobytes() and results[k].tobytes() == r1[0].tobytes(), k
        assert cov[a0:a1].tobytes() == c1.tobytes(), k
        want, wres, _ = TC.statement("shape%d_%d_0" % (a1 - a0, max_tags))
        assert_same("ragged%d[%d]" % (max_tags, k), poses[a0:a1], results[k], want, wres)


def test_entry_points_agree_and_repeat(gpu_detector):
    """host against device form; the same input twice gives the same bytes; d_out and d_results do not depend on d_cov; the
    host form seeding itself is the device form on the seeds of its own localisation; a positive huber with times"""
    b, times = TC.ragged()
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    for huber in (0.0, HUBER):
        first = dv.run(b.seq_start, b.dist, b.sigmas, huber, b.max_iters, times)
        again = dv.run(b.seq_start, b.dist, b.sigmas, huber, b.max_iters, times)
        assert first == again
        rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, huber, b.max_iters, b.seed, times)
        assert rc == 0 and (poses.tobytes(), results.tobytes(), cov.tobytes()) == first
        bare = dv.run(b.seq_start, b.dist, b.sigmas, huber, b.max_iters, times, with_cov=False)
        assert bare[:2] == first[:2] and bare[2] == bytes(len(bare[2]))
        rc, p2, r2, c2 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, huber, b.max_iters, b.seed, times, with_cov=False)
        assert rc == 0 and c2 is None and (p2.tobytes(), r2.tobytes()) == first[:2]
        if huber:   # the robust timed call against the statement at the same threshold, one sequence of it
            a0, a1 = SQ.ranges(b)[3]
            want, wres, _ = TC.run(b.obs[a0:a1], b.rec, b.seed[a0:a1], None, times[a0:a1], b.sigmas, max_iters=b.max_iters, huber=huber)
            assert_same("ragged[3] huber", poses[a0:a1], results[3], want, wres)
    own = gpu_detector.localize(b.obs, b.rec, SC.K, b.dist, SC.TAG)
    seeded = OnDevice(gpu_detector, b.obs, b.rec, own).run(b.seq_start, b.dist, b.sigmas, 0.0, b.max_iters, times)
    rc, p3, r3, c3 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, 0.0, b.max_iters, None, times)
    assert rc == 0 and (p3.tobytes(), r3.tobytes(), c3.tobytes()) == seeded


def test_bad_times_batch(gpu_detector):
    b, times = TC.bad_times_batch()
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed, times)
    assert rc == 0 and results["status"].tolist() == TC.BAD_STATUS
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    assert dv.run(b.seq_start, b.dist, b.sigmas, 0.0, b.max_iters, times) == (poses.tobytes(), results.tobytes(), cov.tobytes())
    want, wres = SR.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, b.seed, *b.sigmas, b.max_iters, times=times)
    for k, (a0, a1) in enumerate(SQ.ranges(b)):
        rc1, p1, r1, c1 = host(gpu_detector, b.obs[a0:a1], [0, a1 - a0], b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed[a0:a1], times[a0:a1])
        assert rc1 == 0 and poses[a0:a1].tobytes() == p1.tobytes() and results[k].tobytes() == r1[0].tobytes(), k
        assert cov[a0:a1].tobytes() == c1.tobytes(), k
        if TC.BAD_STATUS[k] == 0:
            assert_same("bad_times[%d]" % k, poses[a0:a1], results[k], want[a0:a1], wres[k])
            assert (cov["status"][a0:a1] == 0).all()
            continue
        assert results[k].tobytes() == wres[k].tobytes()                   # a status-1 result with status 4
        assert poses[a0:a1].tobytes() == want[a0:a1].tobytes()             # status-1 frames: T identity, seed_slot -1
        assert (poses["status"][a0:a1] == 1).all() and (poses["seed_slot"][a0:a1] == -1).all()
        assert (cov["status"][a0:a1] == 1).all() and not cov["cov"][a0:a1].any() and (cov["dof"][a0:a1] == 0).all()
    # a sequence of one frame needs only a finite time
    obs, rec, seed, dist, _, sig, iters = CASES["shape1_4_0"]
    rc, p, r, c = host(gpu_detector, obs, [0, 1], rec, dist, sig, 0.0, iters, seed, np.array([-7.25]))
    assert rc == 0 and r["status"][0] == 0 and p.tobytes() == device_case(gpu_detector, "shape1_4_0")[0].tobytes()
    for t in (np.nan, np.inf, -np.inf):
        rc, p, r, c = host(gpu_detector, obs, [0, 1], rec, dist, sig, 0.0, iters, seed, np.array([t]))
        assert rc == 0 and r["status"][0] == 4 and p["status"][0] == 1 and c["status"][0] == 1


def gap_on_device(det):
    """(timed on the kept frames, naive, emptied: all frames with the gap emptied), each (poses, result, cov), run once"""
    if "gap" not in _runs:
        obs, rec, seed, _ = TC.gap_scene()
        k = TC.kept_frames()
        s, it = TC.GAP_SIGMAS, SC.MAX_ITERS
        eo, _, es = TC.emptied_gap()
        runs = []
        for o, sd, tm in ((obs[k], seed[k], k.astype(np.float64)), (obs[k], seed[k], None), (eo, es, None)):
            rc, p, r, c = host(det, o, [0, len(o)], rec, None, s, 0.0, it, sd, tm)
            assert rc == 0 and r["status"][0] == 0
            runs.append((p, r[0], c))
        _runs["gap"] = tuple(runs)
    return _runs["gap"]


@pytest.mark.parametrize("name", ["shape5_4_0", "shape65_4_0", "gap"])
def test_covariance_is_the_timed_matrix(gpu_detector, name):
    """d_cov against the timed statement's at the device's own poses, within test_gpu_smooth_cov.py's bar (600 eps kappa)"""
    if name == "gap":
        obs, rec, _, _ = TC.gap_scene()
        k = TC.kept_frames()
        obs, dist, times, sig = obs[k], None, k.astype(np.float64), TC.GAP_SIGMAS
        out, res, cov = gap_on_device(gpu_detector)[0]
    else:
        obs, rec, seed, dist, times, sig, iters = CASES[name]
        out, res, cov = device_case(gpu_detector, name)
    want, A = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig, times=times)
    assert res["status"] == 0 and (want["status"] == 0).all()
    for key in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[key], want[key]), (name, key, cov[key], want[key])
    print("%s: worst scaled covariance error %.3g" % (name, TC.scaled_cov_err(cov["cov"], want["cov"])))
    for f in range(len(out)):
        CK.assert_cov_close(cov["cov"][f], want["cov"][f], A, (name, f))


def test_gap_scene_on_the_device(gpu_detector):
    timed, naive, emptied = gap_on_device(gpu_detector)
    k = TC.kept_frames()
    r = TC.recorded()
    got = TC.gap_rmses(timed[0]["T"], naive[0]["T"])
    e = TC.worst_rel(timed[0]["T"], emptied[0]["T"][k])
    print("gap scene on the device:", {key: "%.6g" % v for key, v in got.items()}, "timed against emptied %.4g (bound %.4g), trials %d / %d / %d" %
          (e, 10 * r["marg_gap"], timed[1]["iterations"], naive[1]["iterations"], emptied[1]["iterations"]))
    assert got["gap_timed_near"] <= r["gap_timed_near"] and got["gap_timed_all"] <= r["gap_timed_all"]
    assert got["gap_naive_near"] >= 1.5 * got["gap_timed_near"]
    assert e <= 10 * r["marg_gap"]


def test_refusals_write_nothing(gpu_detector):
    import torch
    b, times = TC.ragged()
    L = _lib.load()
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    n_seq = len(b.seq_start) - 1
    out = dv.outputs(n_seq, 0xAB)
    keep, fn, ok = dv.args(b.seq_start, b.dist, b.sigmas, HUBER, b.max_iters, out, True, times)
    assert len(ok) == 23 and fn is L.asl_smooth_timed_sequences_device
    nan, inf = float("nan"), float("inf")
    tbytes = 8 * dv.n
    bad = [(17, -1.0), (17, nan), (17, inf), (14, 0.0), (15, nan), (18, 0), (18, 101), (13, 0), (10, None), (12, None), (19, None), (20, None),
           (11, out[0].data_ptr()), (11, out[0].data_ptr() + out[0].numel() - 8), (11, out[2].data_ptr()),
           (11, out[2].data_ptr() + out[2].numel() - 8), (19, keep[3].data_ptr()), (21, keep[3].data_ptr() + tbytes - 8)]
    seed_before, times_before = dv.d_seed.cpu().numpy().tobytes(), keep[3].cpu().numpy().tobytes()
    for k, v in bad:
        a = list(ok)
        a[k] = v
        assert fn(*a) == -1, (k, v)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 0xAB).all() for o in out)
    assert dv.d_seed.cpu().numpy().tobytes() == seed_before and keep[3].cpu().numpy().tobytes() == times_before
    obs, seed, st = np.ascontiguousarray(b.obs), np.ascontiguousarray(b.seed), np.ascontiguousarray(b.seq_start, dtype=np.int32)
    tm = np.ascontiguousarray(times)
    Kc, dc, cam = _camera(b.dist)
    h_out = np.full(dv.n * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    h_res = np.full(n_seq * 64, 0xAB, dtype=np.uint8)
    h_cov = np.full(dv.n * POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    hk = [gpu_detector._h, obs.ctypes.data, dv.n, dv.mt, b.rec.ctypes.data, len(b.rec), *cam, seed.ctypes.data, tm.ctypes.data_as(DP),
          st.ctypes.data_as(IP), n_seq, *b.sigmas, HUBER, b.max_iters, h_out.ctypes.data, h_res.ctypes.data, h_cov.ctypes.data]
    assert len(hk) == 22
    for k, v in [(17, -1.0), (17, nan), (17, inf), (14, 0.0), (18, 101), (13, 0), (12, None), (19, None), (20, None)]:
        a = list(hk)
        a[k] = v
        assert L.asl_smooth_timed_sequences_batch(*a) == -1, (k, v)
    assert (h_out == 0xAB).all() and (h_res == 0xAB).all() and (h_cov == 0xAB).all()
    # and a good call writes
    assert fn(*ok) == 0
    dv.stream.synchronize()
    assert not any((o.cpu().numpy() == 0xAB).all() for o in out)
    assert L.asl_smooth_timed_sequences_batch(*hk) == 0
    assert h_out.tobytes() == out[0].cpu().numpy().tobytes() and h_res.tobytes() == out[1].cpu().numpy().tobytes()
    assert h_cov.tobytes() == out[2].cpu().numpy().tobytes()


def test_python_surface(gpu_detector):
    """Detector.smooth / smooth_sequences(times=...) and smooth_device(times_ptr=...) are the new entry points;
    TagDetector.localize_sequence(s)(times=...) on what detect_host returns; SmoothResult.times and pose_at"""
    import torch
    from aprilslam_amd.localize import TagMap
    from aprilslam_amd.smooth import SmoothResult
    from aprilslam_amd.tag_detector import TagDetector
    obs, rec, seed, dist, times, sig, iters = CASES["shape5_4_5"]
    want = device_case(gpu_detector, "shape5_4_5")
    got = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, with_cov=True, times=times)
    assert got[1].shape == () and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    bare = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, times=times)
    assert len(bare) == 2 and bare[0].tobytes() == want[0].tobytes() and bare[1].tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, times=times[:4])
    b, bt = TC.ragged()
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed, bt)
    many = gpu_detector.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters, seed=b.seed,
                                         with_cov=True, times=bt)
    assert rc == 0 and many[0].tobytes() == poses.tobytes() and many[1].tobytes() == results.tobytes() and many[2].tobytes() == cov.tobytes()
    dev = torch.device("cuda:0")
    d = [CK.dev_bytes(x, dev) for x in (obs, rec, seed, np.ascontiguousarray(times))]
    d_out = torch.zeros(len(obs) * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_detector.smooth_device(d[0].data_ptr(), len(obs), obs.shape[1], d[1].data_ptr(), len(rec), d[2].data_ptr(), d_out.data_ptr(),
                               d_res.data_ptr(), SC.K, dist, SC.TAG, *sig, max_iters=iters, times_ptr=d[3].data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want[0].tobytes() and d_res.cpu().numpy().tobytes() == want[1].tobytes()

    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, id_limit=0)
    cams = [LC.trajectory(520)[i] for i in (0, 1, 4)]       # frames 2 and 3 dropped
    frames = [synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r)[0] for p, r in cams]
    dd, p, npf = td.detector._det.detect_host(np.stack(frames), K=SC.K, dist=np.zeros(4), tag_size=SC.TAG)
    kw = dict(sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2, max_iters=30)
    ft = [0.0, 1.0, 4.0]
    r = td.localize_sequence(dd, p, npf, tm, times=ft, **kw)
    plain = td.localize_sequence(dd, p, npf, tm, **kw)
    unit = td.localize_sequence(dd, p, npf, tm, times=[5.0, 6.0, 7.0], **kw)
    assert isinstance(r, SmoothResult) and r.ok and plain.ok and np.array_equal(r.times, ft) and plain.times is None
    assert unit.poses.tobytes() == plain.poses.tobytes() and r.poses.tobytes() != plain.poses.tobytes()
    assert np.array_equal(r.pose_at(4.0), r.trajectory()[2]) and np.array_equal(r.pose_at(0.0), r.trajectory()[0])
    truth = LC.world_from_camera(*LC.trajectory(520)[2])
    mid = r.pose_at(2.0)
    print("pose_at(2.0): position error to the dropped frame's truth %.4g" % np.linalg.norm(mid[:3, 3] - truth[:3, 3]))
    assert np.abs(mid - SR.pose_at(r.trajectory(), ft, 2.0)).max() <= 1e-14
    with pytest.raises(ValueError):
        r.pose_at(4.5)
    badt = td.localize_sequence(dd, p, npf, tm, times=[0.0, 1.0, 1.0], **kw)
    assert not badt.ok and int(badt.result["status"]) == 4
    two = td.localize_sequences([(dd, p, npf, ft), (dd, p, npf)], tm, **kw)
    assert len(two) == 2 and two[0].poses.tobytes() == r.poses.tobytes() and two[0].result.tobytes() == r.result.tobytes()
    assert two[1].poses.tobytes() == plain.poses.tobytes() and np.array_equal(two[0].times, ft) and two[1].times is None
    both = td.localize_sequences([(dd, p, npf), (dd, p, npf)], tm, **kw)
    assert all(x.poses.tobytes() == plain.poses.tobytes() and x.times is None for x in both)
