"""The robust (Huber) sequence localisation on the device (asl_smooth_robust_sequences_device / _batch: k_smooth_cand<true>,
k_smooth_lin<true>, k_smooth.inc) against the NumPy statement (tests/smooth_ref.py at huber_px > 0) on the cases and recorded figures
of tests/smooth_robust_cases.py, and at huber_px 0 against the plain entry points, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_robust_cases as RC
import smooth_seq_cases as SQ
import solver_checks as CK
from aprilslam_amd import _lib, synth
from aprilslam_amd._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in RC.all_cases()}
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _camera(dist):
    Kc = np.ascontiguousarray(SC.K, dtype=np.float64)
    dc = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64)
    return Kc, dc, (Kc.ctypes.data_as(DP), None if dc is None else dc.ctypes.data_as(DP), 0 if dc is None else len(dc), SC.TAG)


def host(det, obs, start, rec, dist, sigmas, huber, iters, seed, with_cov=True):
    """asl_smooth_robust_sequences_batch (huber None: asl_smooth_sequences_batch) through ctypes, so that huber_px 0.0 reaches
    the new entry point -> (rc, poses, results, cov or None)"""
    L = _lib.load()
    o, sd, st = np.ascontiguousarray(obs), None if seed is None else np.ascontiguousarray(seed), np.ascontiguousarray(start, dtype=np.int32)
    n, mt = o.shape
    Kc, dc, cam = _camera(dist)
    out, res = np.zeros(n, dtype=CAM_POSE_DTYPE), np.zeros(len(st) - 1, dtype=SMOOTH_RESULT_DTYPE)
    cov = np.zeros(n, dtype=POSE_COV_DTYPE) if with_cov else None
    fn, extra = (L.asl_smooth_sequences_batch, ()) if huber is None else (L.asl_smooth_robust_sequences_batch, (float(huber),))
    rc = fn(det._h, o.ctypes.data, n, mt, rec.ctypes.data, len(rec), *cam, None if sd is None else sd.ctypes.data, st.ctypes.data_as(IP), len(st) - 1,
            *sigmas, *extra, iters, out.ctypes.data, res.ctypes.data, None if cov is None else cov.ctypes.data)
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

    def args(self, start, dist, sigmas, huber, iters, out, with_cov):
        st = np.ascontiguousarray(start, dtype=np.int32)
        Kc, dc, cam = _camera(dist)
        keep = (st, Kc, dc)
        extra = () if huber is None else (float(huber),)
        return keep, [self.det._h, self.d_obs.data_ptr(), self.n, self.mt, self.d_map.data_ptr(), self.n_ids, *cam, self.d_seed.data_ptr(),
                      st.ctypes.data_as(IP), len(st) - 1, *sigmas, *extra, iters, out[0].data_ptr(), out[1].data_ptr(),
                      out[2].data_ptr() if with_cov else None, self.stream.cuda_stream]

    def run(self, start, dist, sigmas, huber, iters, with_cov=True):
        L = _lib.load()
        out = self.outputs(len(start) - 1)
        keep, a = self.args(start, dist, sigmas, huber, iters, out, with_cov)
        fn = L.asl_smooth_sequences_device if huber is None else L.asl_smooth_robust_sequences_device
        assert fn(*a) == 0, L.asl_last_error()
        self.stream.synchronize()
        return tuple(o.cpu().numpy().tobytes() for o in out)


_runs = {}


def device_case(det, name):
    """(poses, result, cov) of the host form with d_cov on a case of smooth_robust_cases.all_cases(), run once"""
    if name not in _runs:
        obs, rec, seed, dist, sig, huber, iters = CASES[name]
        rc, out, res, cov = host(det, obs, [0, len(obs)], rec, dist, sig, huber, iters, seed)
        assert rc == 0
        _runs[name] = (out, res[0], cov)
    return _runs[name]


def close(a, b, rel=1e-6):
    return abs(a - b) <= rel * max(1.0, abs(b))


def assert_same(name, got, gres, want, wres):
    """every field of the device's records against the robust statement's"""
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d / %d, cost %.12g / %.12g, n_soft %d / %d" %
          (name, worst, RC.ROBUST_TOL, gres["iterations"], wres["iterations"], gres["cost"], wres["cost"], gres["n_soft"], wres["n_soft"]))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    for k in ("n_frames_data", "n_filled", "n_flipped", "status", "iterations", "n_soft"):
        assert gres[k] == wres[k], (name, k, gres[k], wres[k])
    assert not np.any(gres["reserved"]) and gres["n_soft"] == got["n_rejected"].sum()
    assert worst <= RC.ROBUST_TOL, (name, worst)
    for k in ("rms_px", "rms_seed_px"):
        assert all(close(g, w) for g, w in zip(got[k], want[k])), (name, k)
        assert close(gres[k], wres[k]), (name, k)
    for k in ("cost", "cost_seed"):
        assert close(gres[k], wres[k]), (name, k, gres[k], wres[k])


@pytest.mark.parametrize("shape", RC.SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_device_matches_the_statement(gpu_detector, shape):
    name = "shape%d_%d_%d" % shape
    got, gres, _ = device_case(gpu_detector, name)
    want, wres, _ = RC.statement(name)
    assert gres["status"] == 0 and gres["n_soft"] >= 1
    assert_same(name, got, gres, want, wres)


def test_scene_on_the_device(gpu_detector):
    obs, rec, seed, truth = RC.scene()
    got, gres, _ = device_case(gpu_detector, "scene")
    want, wres, _ = RC.statement("scene")
    r = RC.recorded()
    robust = RC.rmse(got["T"], truth)
    plain, pres = gpu_detector.smooth(obs, rec, SC.K, None, SC.TAG, *SC.NOISE_SIGMAS, max_iters=RC.SCENE_ITERS, seed=seed)
    squared = RC.rmse(plain["T"], truth)
    print("scene: robust %.6g (recorded %.4g), plain %.6g, trials %d / %d, n_soft %d / %d, soft frames %s" %
          (robust, r["scene_rmse_robust"], squared, gres["iterations"], wres["iterations"], gres["n_soft"], wres["n_soft"],
           np.flatnonzero(got["n_rejected"]).tolist()))
    assert gres["status"] == 0 and pres["status"] == 0 and pres["n_soft"] == 0 and not plain["n_rejected"].any()
    assert robust <= r["scene_rmse_robust"]
    assert squared >= 10 * robust
    assert gres["n_soft"] == wres["n_soft"] == r["scene_soft"] and np.array_equal(got["n_rejected"], want["n_rejected"])
    from aprilslam_amd.smooth import SmoothResult
    sr = SmoothResult(got, gres, seed)
    assert sr.soft[RC.SCENE_FRAMES].all() and sr.n_soft == r["scene_soft"]
    assert_same("scene", got, gres, want, wres)


PLAIN = {c[0]: c[1:] for c in SC.all_cases()}


@pytest.mark.parametrize("name", list(PLAIN))
def test_huber_zero_is_the_plain_call(gpu_detector, name):
    """huber_px 0 through the new entry points: the bytes of asl_smooth_sequences_batch / _device, with and without d_cov"""
    obs, rec, seed, dist, sig, iters = PLAIN[name]
    start = [0, len(obs)]
    dv = OnDevice(gpu_detector, obs, rec, seed)
    for with_cov in (True, False):
        rc0, p0, r0, c0 = host(gpu_detector, obs, start, rec, dist, sig, None, iters, seed, with_cov)
        rc1, p1, r1, c1 = host(gpu_detector, obs, start, rec, dist, sig, 0.0, iters, seed, with_cov)
        assert rc0 == 0 and rc1 == 0 and p0.tobytes() == p1.tobytes() and r0.tobytes() == r1.tobytes() and r1["n_soft"] == 0
        assert (c0 is None and c1 is None) or c0.tobytes() == c1.tobytes()
        d0, d1 = dv.run(start, dist, sig, None, iters, with_cov), dv.run(start, dist, sig, 0.0, iters, with_cov)
        assert d0 == d1 and d0[0] == p0.tobytes() and d0[1] == r0.tobytes()
        assert d0[2] == (c0.tobytes() if with_cov else bytes(len(d0[2])))


def test_huber_zero_is_the_plain_call_on_a_batch(gpu_detector):
    b = SQ.failures()
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    for with_cov in (True, False):
        rc0, p0, r0, c0 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, None, b.max_iters, b.seed, with_cov)
        rc1, p1, r1, c1 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, 0.0, b.max_iters, b.seed, with_cov)
        assert rc0 == 0 and rc1 == 0 and p0.tobytes() == p1.tobytes() and r0.tobytes() == r1.tobytes()
        assert (c0 is None and c1 is None) or c0.tobytes() == c1.tobytes()
        assert dv.run(b.seq_start, b.dist, b.sigmas, None, b.max_iters, with_cov) == dv.run(b.seq_start, b.dist, b.sigmas, 0.0, b.max_iters, with_cov)
    assert r0["status"].tolist() == SQ.FAILURES_STATUS


@pytest.mark.parametrize("which", ["ragged", "mixed"])
def test_each_sequence_of_a_batch_is_the_call_alone(gpu_detector, which):
    b = RC.ragged() if which == "ragged" else RC.mixed()
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, b.huber, b.max_iters, b.seed)
    assert rc == 0
    for k, (a0, a1) in enumerate(SQ.ranges(b)):
        rc1, p1, r1, c1 = host(gpu_detector, b.obs[a0:a1], [0, a1 - a0], b.rec, b.dist, b.sigmas, b.huber, b.max_iters, b.seed[a0:a1])
        assert rc1 == 0 and poses[a0:a1].tobytes() == p1.tobytes() and results[k].tobytes() == r1[0].tobytes(), (which, k)
        assert cov[a0:a1].tobytes() == c1.tobytes(), (which, k)
        want, wres, _ = RC.batch_statement(which, k)
        if wres["status"] == 0:
            assert_same("%s[%d]" % (which, k), poses[a0:a1], results[k], want, wres)
        else:
            assert results[k]["status"] == wres["status"] and results[k]["iterations"] == wres["iterations"] and results[k]["n_soft"] == wres["n_soft"]
            assert np.array_equal(poses["status"][a0:a1], want["status"]) and np.array_equal(poses["n_rejected"][a0:a1], want["n_rejected"])
    if which == "mixed":
        assert results["status"].tolist() == RC.MIXED_STATUS and results["n_soft"][0] == 0 and results["n_soft"][1] >= 1
        for (a0, a1), st in zip(SQ.ranges(b), RC.MIXED_COV_STATUS):
            assert (cov["status"][a0:a1] == st).all()
    else:
        assert (results["status"] == 0).all() and (results["n_soft"] >= 1).all() and (cov["status"] == 0).all()


def test_entry_points_agree_and_repeat(gpu_detector):
    """host against device form; the same input twice gives the same bytes; d_out and d_results do not depend on d_cov; the
    host form seeding itself is the device form on the seeds of its own localisation"""
    b = RC.ragged()
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    first = dv.run(b.seq_start, b.dist, b.sigmas, b.huber, b.max_iters)
    again = dv.run(b.seq_start, b.dist, b.sigmas, b.huber, b.max_iters)
    assert first == again
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, b.huber, b.max_iters, b.seed)
    assert rc == 0 and (poses.tobytes(), results.tobytes(), cov.tobytes()) == first
    bare = dv.run(b.seq_start, b.dist, b.sigmas, b.huber, b.max_iters, with_cov=False)
    assert bare[:2] == first[:2] and bare[2] == bytes(len(bare[2]))
    rc, p2, r2, c2 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, b.huber, b.max_iters, b.seed, with_cov=False)
    assert rc == 0 and c2 is None and (p2.tobytes(), r2.tobytes()) == first[:2]
    own = gpu_detector.localize(b.obs, b.rec, SC.K, b.dist, SC.TAG)
    seeded = OnDevice(gpu_detector, b.obs, b.rec, own).run(b.seq_start, b.dist, b.sigmas, b.huber, b.max_iters)
    rc, p3, r3, c3 = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, b.huber, b.max_iters, None)
    assert rc == 0 and (p3.tobytes(), r3.tobytes(), c3.tobytes()) == seeded


@pytest.mark.parametrize("name", ["shape5_4_0", "shape3_20_0", "shape65_4_0", "scene"])
def test_covariance_is_the_weighted_matrix(gpu_detector, name):
    """d_cov against the robust statement's at the device's own poses, within test_gpu_smooth_cov.py's bar (600 eps kappa)"""
    obs, rec, seed, dist, sig, huber, iters = CASES[name]
    out, res, cov = device_case(gpu_detector, name)
    want = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig, huber)[0]
    assert res["status"] == 0 and (want["status"] == 0).all()
    for k in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[k], want[k]), (name, k, cov[k], want[k])
    _, A = SV.dense_marginals(obs, rec, SC.K, dist, SC.TAG, out, *sig, huber)
    worst = 0.0
    for f in range(len(out)):
        s = np.sqrt(np.diag(want["cov"][f]))
        worst = max(worst, float((np.abs(cov["cov"][f] - want["cov"][f]) / np.outer(s, s)).max()))
    print("%s: worst scaled covariance error %.3g" % (name, worst))
    for f in range(len(out)):
        CK.assert_cov_close(cov["cov"][f], want["cov"][f], A, (name, f))


def test_refusals_write_nothing(gpu_detector):
    import torch
    b = RC.ragged()
    L = _lib.load()
    dv = OnDevice(gpu_detector, b.obs, b.rec, b.seed)
    n_seq = len(b.seq_start) - 1
    out = dv.outputs(n_seq, 0xAB)
    keep, ok = dv.args(b.seq_start, b.dist, b.sigmas, b.huber, b.max_iters, out, True)
    assert len(ok) == 22
    nan, inf = float("nan"), float("inf")
    bad = [(16, -1.0), (16, nan), (16, inf), (16, -inf), (13, 0.0), (17, 0), (12, 0), (10, None), (19, None)]
    seed_before = dv.d_seed.cpu().numpy().tobytes()
    for k, v in bad:
        a = list(ok)
        a[k] = v
        assert L.asl_smooth_robust_sequences_device(*a) == -1, (k, v)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 0xAB).all() for o in out) and dv.d_seed.cpu().numpy().tobytes() == seed_before
    obs, seed, st = np.ascontiguousarray(b.obs), np.ascontiguousarray(b.seed), np.ascontiguousarray(b.seq_start, dtype=np.int32)
    Kc, dc, cam = _camera(b.dist)
    h_out = np.full(dv.n * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    h_res = np.full(n_seq * 64, 0xAB, dtype=np.uint8)
    h_cov = np.full(dv.n * POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    hk = [gpu_detector._h, obs.ctypes.data, dv.n, dv.mt, b.rec.ctypes.data, len(b.rec), *cam, seed.ctypes.data, st.ctypes.data_as(IP), n_seq,
          *b.sigmas, b.huber, b.max_iters, h_out.ctypes.data, h_res.ctypes.data, h_cov.ctypes.data]
    assert len(hk) == 21
    for k, v in [(16, -1.0), (16, nan), (16, inf), (13, 0.0), (17, 101), (12, 0), (19, None)]:
        a = list(hk)
        a[k] = v
        assert L.asl_smooth_robust_sequences_batch(*a) == -1, (k, v)
    assert (h_out == 0xAB).all() and (h_res == 0xAB).all() and (h_cov == 0xAB).all()
    # and a good call writes
    assert L.asl_smooth_robust_sequences_device(*ok) == 0
    dv.stream.synchronize()
    assert not any((o.cpu().numpy() == 0xAB).all() for o in out)
    assert L.asl_smooth_robust_sequences_batch(*hk) == 0
    assert h_out.tobytes() == out[0].cpu().numpy().tobytes() and h_res.tobytes() == out[1].cpu().numpy().tobytes()
    assert h_cov.tobytes() == out[2].cpu().numpy().tobytes()


def test_python_surface(gpu_detector):
    """Detector.smooth / smooth_sequences(huber_px=...) are the new entry points; TagDetector.localize_sequence(s)(huber_px=...)
    on what detect_host returns"""
    from aprilslam_amd.localize import TagMap
    from aprilslam_amd.smooth import SmoothResult
    from aprilslam_amd.tag_detector import TagDetector
    obs, rec, seed, dist, sig, huber, iters = CASES["shape5_4_5"]
    want = device_case(gpu_detector, "shape5_4_5")
    got = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, with_cov=True, huber_px=huber)
    assert got[1].shape == () and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    bare = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, huber_px=huber)
    assert len(bare) == 2 and bare[0].tobytes() == want[0].tobytes() and bare[1].tobytes() == want[1].tobytes()
    b = RC.ragged()
    rc, poses, results, cov = host(gpu_detector, b.obs, b.seq_start, b.rec, b.dist, b.sigmas, b.huber, b.max_iters, b.seed)
    many = gpu_detector.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters, seed=b.seed,
                                         with_cov=True, huber_px=b.huber)
    assert rc == 0 and many[0].tobytes() == poses.tobytes() and many[1].tobytes() == results.tobytes() and many[2].tobytes() == cov.tobytes()
    with pytest.raises(_lib.AslError):
        gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, huber_px=-1.0)

    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, id_limit=0)
    cams = LC.trajectory(520)[:3]
    frames = [synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r)[0] for p, r in cams]
    d, p, npf = td.detector._det.detect_host(np.stack(frames), K=SC.K, dist=np.zeros(4), tag_size=SC.TAG)
    d = d.copy()
    d["corners"][0, 0] += np.float32(9.0)       # one slipped corner in frame 0
    kw = dict(sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2, max_iters=30)
    r = td.localize_sequence(d, p, npf, tm, huber_px=1.0, **kw)
    plain = td.localize_sequence(d, p, npf, tm, **kw)
    assert isinstance(r, SmoothResult) and r.ok and plain.ok and plain.n_soft == 0 and not plain.soft.any()
    assert r.n_soft >= 1 and r.soft[0] and r.n_soft == r.poses["n_rejected"].sum()
    truth = [LC.world_from_camera(*c) for c in cams]
    err = lambda res: np.linalg.norm(res.trajectory()[0][:3, 3] - truth[0][:3, 3])
    print("slipped corner: frame 0 position error robust %.4g, plain %.4g, n_soft %d" % (err(r), err(plain), r.n_soft))
    assert err(r) < err(plain)
    two = td.localize_sequences([(d, p, npf), (d, p, npf)], tm, huber_px=1.0, **kw)
    assert len(two) == 2 and all(x.poses.tobytes() == r.poses.tobytes() and x.result.tobytes() == r.result.tobytes() for x in two)
