"""The rig sequence localisation on the device (asl_smooth_rig_sequences_device / _batch: k_smooth_rig_cand and k_smooth_rig_lin
over LocRig in k_smooth.inc) against the NumPy statement (tests/smooth_ref.py) on the cases and recorded figures of
tests/smooth_rig_cases.py; one camera at E = I against asl_smooth_timed_sequences_device; the identities that need no
statement; the covariance; the refusals; the Python surface."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_ref as SR
import smooth_rig_cases as GC
import solver_checks as CK
from aprilslam_amd import _lib
from aprilslam_amd._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE
from aprilslam_amd.rig import Rig, RigCamera
from aprilslam_amd.smooth import SmoothResult

pytestmark = pytest.mark.gpu

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def host(det, obs, rec, rig, seed, sigmas, huber, iters, start=None, times=None, with_cov=True):
    """asl_smooth_rig_sequences_batch through ctypes -> (rc, poses, results, cov or None)"""
    o, tab = np.ascontiguousarray(obs), _lib._rig_records(rig)
    n_cams, n, mt = o.shape
    sd = None if seed is None else np.ascontiguousarray(seed)
    st = np.ascontiguousarray([0, n] if start is None else start, dtype=np.int32)
    tm = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
    out, res = np.zeros(n, dtype=CAM_POSE_DTYPE), np.zeros(len(st) - 1, dtype=SMOOTH_RESULT_DTYPE)
    cov = np.zeros(n, dtype=POSE_COV_DTYPE) if with_cov else None
    rc = _lib.load().asl_smooth_rig_sequences_batch(det._h, o.ctypes.data, n_cams, n, mt, rec.ctypes.data, len(rec), tab.ctypes.data, GC.TAG,
                                                    None if sd is None else sd.ctypes.data, None if tm is None else tm.ctypes.data_as(DP),
                                                    st.ctypes.data_as(IP), len(st) - 1, *sigmas, float(huber), iters, out.ctypes.data,
                                                    res.ctypes.data, None if cov is None else cov.ctypes.data)
    return rc, out, res, cov


class OnDevice:
    """a rig block on device buffers; run(): one enqueue on a stream of its own, then the outputs' bytes"""

    def __init__(self, det, obs, rec, rig, seed):
        import torch
        self.torch, self.det, self.dev = torch, det, torch.device("cuda:0")
        self.n_cams, self.n, self.mt = obs.shape
        self.n_ids = len(rec)
        self.d_obs, self.d_map, self.d_seed = CK.dev_bytes(obs, self.dev), CK.dev_bytes(rec, self.dev), CK.dev_bytes(seed, self.dev)
        self.d_rig = CK.dev_bytes(_lib._rig_records(rig), self.dev)
        self.stream = torch.cuda.Stream(self.dev)

    def outputs(self, n_seq, fill=0):
        t = self.torch
        out = [t.full((size,), fill, dtype=t.uint8, device=self.dev)
               for size in (self.n * CAM_POSE_DTYPE.itemsize, n_seq * SMOOTH_RESULT_DTYPE.itemsize, self.n * POSE_COV_DTYPE.itemsize)]
        t.cuda.synchronize()
        return out

    def args(self, start, sigmas, huber, iters, out, with_cov, times=None):
        st = np.ascontiguousarray([0, self.n] if start is None else start, dtype=np.int32)
        d_times = None if times is None else CK.dev_bytes(np.ascontiguousarray(times, dtype=np.float64), self.dev)
        self.torch.cuda.synchronize()
        return (st, d_times), [self.det._h, self.d_obs.data_ptr(), self.n_cams, self.n, self.mt, self.d_map.data_ptr(), self.n_ids,
                               self.d_rig.data_ptr(), GC.TAG, self.d_seed.data_ptr(), None if d_times is None else d_times.data_ptr(),
                               st.ctypes.data_as(IP), len(st) - 1, *sigmas, float(huber), iters, out[0].data_ptr(), out[1].data_ptr(),
                               out[2].data_ptr() if with_cov else None, self.stream.cuda_stream]

    def run(self, start, sigmas, huber, iters, times=None, with_cov=True, fill=0):
        out = self.outputs(1 if start is None else len(start) - 1, fill)
        keep, a = self.args(start, sigmas, huber, iters, out, with_cov, times)
        assert _lib.load().asl_smooth_rig_sequences_device(*a) == 0, _lib.load().asl_last_error()
        self.stream.synchronize()
        return tuple(o.cpu().numpy().tobytes() for o in out)


_runs = {}


def device_case(det, name, huber=0.0):
    """(poses, result, cov) of the host form with cov on a case of smooth_rig_cases.all_cases(), run once"""
    if (name, huber) not in _runs:
        _, obs, rec, rig, seed, sig, iters, times = GC.case(name)
        rc, out, res, cov = host(det, obs, rec, rig, seed, sig, huber, iters, times=times)
        assert rc == 0, _lib.load().asl_last_error()
        _runs[(name, huber)] = (out, res[0], cov)
    return _runs[(name, huber)]


def close(a, b, rel=1e-6):
    return abs(a - b) <= rel * max(1.0, abs(b))


def assert_same(name, got, gres, want, wres, tol=GC.DEVICE_TOL):
    """every field of the device's records against the statement's"""
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d / %d, cost %.12g / %.12g" %
          (name, worst, tol, gres["iterations"], wres["iterations"], gres["cost"], wres["cost"]))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    for k in ("n_frames_data", "n_filled", "n_flipped", "status", "iterations", "n_soft"):
        assert gres[k] == wres[k], (name, k, gres[k], wres[k])
    assert not np.any(gres["reserved"]) and gres["n_soft"] == got["n_rejected"].sum()
    assert worst <= tol, (name, worst)
    for k in ("rms_px", "rms_seed_px"):
        assert all(close(g, w) for g, w in zip(got[k], want[k])), (name, k)
        assert close(gres[k], wres[k]), (name, k)
    for k in ("cost", "cost_seed"):
        assert close(gres[k], wres[k]), (name, k, gres[k], wres[k])


@pytest.mark.parametrize("huber", [0.0, GC.HUBER_PX])
@pytest.mark.parametrize("name", GC.COMPARE)
def test_device_matches_the_statement(gpu_detector, name, huber):
    got, gres, _ = device_case(gpu_detector, name, huber)
    want, wres, _ = GC.statement(name, huber)
    assert_same("%s huber %g" % (name, huber), got, gres, want, wres)


def test_flip_goes_through_the_mounting(gpu_detector):
    """the chain's first decision on the device: B of a frame whose one slot is in camera 1, at COMPARE_ITERS against the statement"""
    _, obs, rec, rig, seed, sig, _, _ = GC.case("flip")
    rc, got, gres, _ = host(gpu_detector, obs, rec, rig, seed, sig, 0.0, GC.COMPARE_ITERS)
    want, wres, _ = SR.smooth_rig(obs, rec, rig, GC.TAG, seed, *sig, GC.COMPARE_ITERS)
    assert rc == 0 and int(wres["n_flipped"]) == len(GC.FLIP_FRAMES)
    assert_same("flip at %d trials" % GC.COMPARE_ITERS, got, gres[0], want, wres)


def test_scenes_at_full_iterations(gpu_detector):
    fig, rec = GC.figures(lambda name, huber: device_case(gpu_detector, name, huber)[0]), GC.recorded()
    print("scenes on the device:", {k: "%.6g" % v for k, v in fig.items()}, "recorded:", rec)
    for k in ("holes_end_err", "holes_mid_err", "flip_margin", "noise_rmse_smooth", "outlier_rmse_huber"):
        assert fig[k] <= rec[k], (k, fig[k], rec[k])
    assert fig["outlier_rmse_plain"] > 2 * fig["outlier_rmse_huber"]
    poses, res, _ = device_case(gpu_detector, "holes")
    assert poses["status"].tolist() == [6, 0, 0, 6, 0, 0, 6] and res["n_filled"] == 3 and res["status"] == 0
    assert poses["n_tags"].tolist() == GC.statement("holes")[0]["n_tags"].tolist()
    poses, res, _ = device_case(gpu_detector, "flip")
    assert res["n_flipped"] == len(GC.FLIP_FRAMES) and all(poses["seed_slot"][f] == 1 + SR.FLIPPED for f in GC.FLIP_FRAMES)
    poses, res, _ = device_case(gpu_detector, "outliers", GC.HUBER_PX)
    assert poses["n_rejected"][GC.OUTLIER_SLIP[1]] >= 1 and poses["n_rejected"][GC.OUTLIER_SWAP[1]] >= 1
    for name in ("noise", "outliers"):       # rig_huber_px 0: nothing is soft
        poses, res, _ = device_case(gpu_detector, name)
        assert res["n_soft"] == 0 and not poses["n_rejected"].any()


@pytest.mark.parametrize("shape", [(1, 1, 0), (2, 4, 0), (5, 1, 0), (5, 4, 5), (64, 4, 0), (65, 1, 0)], ids=lambda s: "%d_%d_%d" % s)
@pytest.mark.parametrize("huber", [0.0, GC.HUBER_PX])
def test_one_camera_at_identity_against_the_single_camera_entry_point(gpu_detector, shape, huber):
    """asl_smooth_timed_sequences_device (d_times NULL) on the same frames: integer fields equal, T within DEVICE_TOL; no byte
    identity, as for the localisation (test_gpu_rig.py)"""
    import torch
    obs, rec, seed, dist = SC.shape(*shape)
    n, mt = obs.shape
    solo = Rig([RigCamera(SC.K, dist, np.eye(4))])
    dv = OnDevice(gpu_detector, obs[None], rec, solo, seed)
    got = dv.run(None, SC.SHAPE_SIGMAS, huber, SC.COMPARE_ITERS, with_cov=False)
    out = dv.outputs(1)
    Kc = np.ascontiguousarray(SC.K)
    dc = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64)
    st = np.array([0, n], dtype=np.int32)
    rc = _lib.load().asl_smooth_timed_sequences_device(gpu_detector._h, dv.d_obs.data_ptr(), n, mt, dv.d_map.data_ptr(), len(rec), Kc.ctypes.data_as(DP),
                                                       None if dc is None else dc.ctypes.data_as(DP), 0 if dc is None else len(dc), SC.TAG,
                                                       dv.d_seed.data_ptr(), None, st.ctypes.data_as(IP), 1, *SC.SHAPE_SIGMAS, float(huber),
                                                       SC.COMPARE_ITERS, out[0].data_ptr(), out[1].data_ptr(), None, dv.stream.cuda_stream)
    assert rc == 0
    dv.stream.synchronize()
    torch.cuda.synchronize()
    one = out[0].cpu().numpy().view(CAM_POSE_DTYPE), out[1].cpu().numpy().view(SMOOTH_RESULT_DTYPE)[0]
    rig = np.frombuffer(got[0], dtype=CAM_POSE_DTYPE), np.frombuffer(got[1], dtype=SMOOTH_RESULT_DTYPE)[0]
    assert_same("one camera %s huber %g" % (shape, huber), rig[0], rig[1], one[0], one[1])


def test_each_sequence_is_the_call_alone(gpu_detector):
    """the three sequences of 1, 2 and 65 frames: poses, result and cov of each, byte for byte, the 0xAB prefill included"""
    obs, rec, rig, seed = GC.three_sequences()
    start = GC.SEQ_START
    for huber in (0.0, GC.HUBER_PX):
        dv = OnDevice(gpu_detector, obs, rec, rig, seed)
        p, r, c = dv.run(start, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, fill=0xAB)
        for k, (a, b) in enumerate(zip(start[:-1], start[1:])):
            one = OnDevice(gpu_detector, obs[:, a:b], rec, rig, seed[a:b])
            p1, r1, c1 = one.run(None, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, fill=0xAB)
            ps, cs = CAM_POSE_DTYPE.itemsize, POSE_COV_DTYPE.itemsize
            assert p[a * ps:b * ps] == p1 and r[64 * k:64 * k + 64] == r1 and c[a * cs:b * cs] == c1, (huber, k)
        want, wres = SR.smooth_rig_sequences(obs, start, rec, rig, GC.TAG, seed, *GC.SHAPE_SIGMAS, GC.COMPARE_ITERS, huber_px=huber)
        got, gres = np.frombuffer(p, dtype=CAM_POSE_DTYPE), np.frombuffer(r, dtype=SMOOTH_RESULT_DTYPE)
        for k, (a, b) in enumerate(zip(start[:-1], start[1:])):
            assert_same("three_sequences[%d] huber %g" % (k, huber), got[a:b], gres[k], want[a:b], wres[k])


def test_entry_points_agree_and_repeat(gpu_detector):
    """d_frame_times NULL and times c + f; host against device form; the same input twice; d_out and d_results do not depend
    on d_cov; the host form seeding itself is the device form on the seeds of the rig localisation"""
    obs, rec, rig, seed = GC.three_sequences()
    start = GC.SEQ_START
    unit = np.concatenate([5.0 + np.arange(b - a) for a, b in zip(start[:-1], start[1:])])
    dv = OnDevice(gpu_detector, obs, rec, rig, seed)
    for huber in (0.0, GC.HUBER_PX):
        first = dv.run(start, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS)
        assert dv.run(start, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS) == first
        assert dv.run(start, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, times=unit) == first
        rc, p, r, c = host(gpu_detector, obs, rec, rig, seed, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, start)
        assert rc == 0 and (p.tobytes(), r.tobytes(), c.tobytes()) == first
        rc, p, r, c = host(gpu_detector, obs, rec, rig, seed, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, start, times=unit)
        assert rc == 0 and (p.tobytes(), r.tobytes(), c.tobytes()) == first
        bare = dv.run(start, GC.SHAPE_SIGMAS, huber, GC.COMPARE_ITERS, with_cov=False)
        assert bare[:2] == first[:2] and bare[2] == bytes(len(bare[2]))
        if huber == 0.0:
            assert not np.frombuffer(first[1], dtype=SMOOTH_RESULT_DTYPE)["n_soft"].any()
    own = gpu_detector.localize_rig(obs, rec, rig, GC.TAG)
    seeded = OnDevice(gpu_detector, obs, rec, rig, own).run(start, GC.SHAPE_SIGMAS, 0.0, GC.COMPARE_ITERS)
    rc, p, r, c = host(gpu_detector, obs, rec, rig, None, GC.SHAPE_SIGMAS, 0.0, GC.COMPARE_ITERS, start)
    assert rc == 0 and (p.tobytes(), r.tobytes(), c.tobytes()) == seeded


@pytest.mark.parametrize("name,huber", [("shape3_5_64", 0.0), ("gap", 0.0), ("mixed_models", GC.HUBER_PX)])
def test_covariance_is_the_statements(gpu_detector, name, huber):
    """d_cov against smooth_cov_ref.marginals of the rig statement's blocks at the device's own poses (600 eps kappa)"""
    _, obs, rec, rig, seed, sig, iters, times = GC.case(name)
    out, res, cov = device_case(gpu_detector, name, huber)
    want, A = SV.smooth_rig_cov(obs, rec, rig, GC.TAG, out, res, *sig, times=times, huber_px=huber)
    assert res["status"] == 0 and (want["status"] == 0).all()
    for key in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[key], want[key]), (name, key, cov[key], want[key])
    for f in range(len(out)):
        CK.assert_cov_close(cov["cov"][f], want["cov"][f], A, (name, f))


def test_covariance_statuses(gpu_detector):
    """2: no frame has a tag (the seeds alone give no information); 1: nothing to solve, and a failed solve"""
    obs, rec, rig, seed = GC.shape(2, 3, 2)
    rc, p, r, c = host(gpu_detector, GC.empty(obs, range(2)), rec, rig, seed, GC.SHAPE_SIGMAS, 0.0, GC.COMPARE_ITERS)
    assert rc == 0 and r["status"][0] == 0 and (p["status"] == 6).all() and (c["status"] == 2).all() and not c["cov"].any()
    _, _, cov = device_case(gpu_detector, "no_posed")
    assert (cov["status"] == 1).all() and not cov["cov"].any() and (cov["dof"] == 0).all()
    behind = seed[:1].copy()
    behind["T"][0] = behind["T"][0] @ np.diag([1.0, -1.0, -1.0, 1.0])       # every corner behind its camera: never positive definite
    rc, p, r, c = host(gpu_detector, obs[:, :1], rec, rig, behind, GC.SHAPE_SIGMAS, 0.0, 4)
    assert rc == 0 and r["status"][0] == SR.NOT_POSITIVE_DEFINITE and p["status"][0] == 4 and c["status"][0] == 1


def test_refusals_write_nothing(gpu_detector):
    import torch
    obs, rec, rig, seed = GC.three_sequences()
    L = _lib.load()
    fn = L.asl_smooth_rig_sequences_device
    dv = OnDevice(gpu_detector, obs, rec, rig, seed)
    out = dv.outputs(3, 0xAB)
    keep, ok = dv.args(GC.SEQ_START, GC.SHAPE_SIGMAS, GC.HUBER_PX, GC.COMPARE_ITERS, out, True, np.arange(dv.n, dtype=np.float64))
    assert len(ok) == 22
    nan, inf = float("nan"), float("inf")
    bent = rig.as_records().copy()
    bent["E"][1][0, 0] += 1e-3                                              # not a rotation
    d_bent = CK.dev_bytes(bent, dv.dev)
    nine = CK.dev_bytes(np.zeros(9 * dv.n * 32, dtype=_lib.OBS_DTYPE), dv.dev)
    torch.cuda.synchronize()
    bad = [[(2, 0)], [(2, 17)], [(2, 9), (4, 32), (1, nine.data_ptr())], [(7, d_bent.data_ptr())], [(7, None)],
           [(16, -1.0)], [(16, nan)], [(16, inf)], [(13, 0.0)], [(14, nan)], [(17, 0)], [(17, 101)], [(12, 0)], [(9, None)], [(11, None)],
           [(18, None)], [(19, None)], [(1, None)], [(5, None)], [(4, 0)], [(4, 257)], [(6, 0)], [(3, 0)], [(8, 0.0)],
           [(10, out[0].data_ptr())], [(18, dv.d_seed.data_ptr())], [(20, out[0].data_ptr())]]
    seed_before = dv.d_seed.cpu().numpy().tobytes()
    for change in bad:
        a = list(ok)
        for k, v in change:
            a[k] = v
        assert fn(*a) == -1, change
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 0xAB).all() for o in out) and dv.d_seed.cpu().numpy().tobytes() == seed_before
    o, sd, st, tab = np.ascontiguousarray(obs), np.ascontiguousarray(seed), np.ascontiguousarray(GC.SEQ_START, dtype=np.int32), rig.as_records()
    tm = np.arange(dv.n, dtype=np.float64)
    h_out = np.full(dv.n * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    h_res = np.full(3 * 64, 0xAB, dtype=np.uint8)
    h_cov = np.full(dv.n * POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    hk = [gpu_detector._h, o.ctypes.data, dv.n_cams, dv.n, dv.mt, rec.ctypes.data, len(rec), tab.ctypes.data, GC.TAG, sd.ctypes.data,
          tm.ctypes.data_as(DP), st.ctypes.data_as(IP), 3, *GC.SHAPE_SIGMAS, GC.HUBER_PX, GC.COMPARE_ITERS, h_out.ctypes.data, h_res.ctypes.data,
          h_cov.ctypes.data]
    assert len(hk) == 21
    big = np.zeros(9 * dv.n * 32, dtype=_lib.OBS_DTYPE)
    for change in [[(2, 0)], [(2, 17)], [(2, 9), (4, 32), (1, big.ctypes.data)], [(7, bent.ctypes.data)], [(7, None)], [(16, -1.0)], [(13, 0.0)],
                   [(17, 101)], [(12, 0)], [(11, None)], [(18, None)], [(19, None)]]:
        a = list(hk)
        for k, v in change:
            a[k] = v
        assert L.asl_smooth_rig_sequences_batch(*a) == -1, change
    assert (h_out == 0xAB).all() and (h_res == 0xAB).all() and (h_cov == 0xAB).all()
    # and a good call writes
    assert fn(*ok) == 0
    dv.stream.synchronize()
    assert not any((x.cpu().numpy() == 0xAB).all() for x in out)
    assert L.asl_smooth_rig_sequences_batch(*hk) == 0
    assert h_out.tobytes() == out[0].cpu().numpy().tobytes() and h_res.tobytes() == out[1].cpu().numpy().tobytes()
    assert h_cov.tobytes() == out[2].cpu().numpy().tobytes()


def test_python_surface(gpu_detector):
    """Detector.smooth_rig / smooth_rig_device and Rig.localize_sequence(s) return the bytes of the ctypes call"""
    import torch
    _, obs, rec, rig, seed, sig, iters, times = GC.case("gap")
    want = device_case(gpu_detector, "gap", GC.HUBER_PX)
    got = gpu_detector.smooth_rig(obs, rec, rig, GC.TAG, *sig, max_iters=iters, seed=seed, times=times, huber_px=GC.HUBER_PX, with_cov=True)
    assert got[1].shape == () and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    r = rig.localize_sequence(gpu_detector, obs, rec, GC.TAG, *sig, max_iters=iters, seed=seed, times=times, huber_px=GC.HUBER_PX, with_cov=True)
    assert isinstance(r, SmoothResult) and r.ok and r.poses.tobytes() == want[0].tobytes() and r.result.tobytes() == want[1].tobytes()
    assert r.cov_records.tobytes() == want[2].tobytes() and np.array_equal(r.times, times) and r.cov.shape == (len(seed), 6, 6)
    assert np.array_equal(r.pose_at(times[2]), r.trajectory()[2]) and r.filled.sum() == 1 and not r.flipped.any() and r.soft.sum() == r.n_soft == 0
    bare = rig.localize_sequence(gpu_detector, obs, rec, GC.TAG, *sig, max_iters=iters, seed=seed, times=times, huber_px=GC.HUBER_PX)
    assert bare.cov_records is None and bare.poses.tobytes() == want[0].tobytes()
    with pytest.raises(ValueError):
        rig.localize_sequence(gpu_detector, obs[:1], rec, GC.TAG)
    obs3, rec3, rig3, seed3 = GC.three_sequences()
    rc, p, res, c = host(gpu_detector, obs3, rec3, rig3, seed3, GC.SHAPE_SIGMAS, 0.0, GC.COMPARE_ITERS, GC.SEQ_START)
    many = rig3.localize_sequences(gpu_detector, obs3, GC.SEQ_START, rec3, GC.TAG, *GC.SHAPE_SIGMAS, max_iters=GC.COMPARE_ITERS, seed=seed3, with_cov=True)
    assert rc == 0 and len(many) == 3
    for k, (a, b) in enumerate(zip(GC.SEQ_START[:-1], GC.SEQ_START[1:])):
        assert many[k].poses.tobytes() == p[a:b].tobytes() and many[k].result.tobytes() == res[k].tobytes()
        assert many[k].cov_records.tobytes() == c[a:b].tobytes()
    dev = torch.device("cuda:0")
    d = [CK.dev_bytes(x, dev) for x in (obs, rec, rig.as_records(), seed, np.ascontiguousarray(times))]
    d_out = torch.zeros(len(seed) * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_cov = torch.zeros(len(seed) * POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_detector.smooth_rig_device(d[0].data_ptr(), obs.shape[0], obs.shape[1], obs.shape[2], d[1].data_ptr(), len(rec), d[2].data_ptr(),
                                   d[3].data_ptr(), d_out.data_ptr(), d_res.data_ptr(), GC.TAG, *sig, max_iters=iters, times_ptr=d[4].data_ptr(),
                                   huber_px=GC.HUBER_PX, cov_ptr=d_cov.data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want[0].tobytes() and d_res.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_cov.cpu().numpy().tobytes() == want[2].tobytes()
