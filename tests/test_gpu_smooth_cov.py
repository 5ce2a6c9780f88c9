"""The covariance of the smoothed sequence poses on the device (asl_smooth_cov_frames_device / asl_smooth_cov_batch,
k_smooth_cov in k_smooth.inc) against the NumPy statement (tests/smooth_cov_ref.py), always at the device's own returned
poses, on the cases and recorded figures of tests/smooth_cov_cases.py."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_cov_cases as VC
import smooth_cov_ref as SV
import solver_checks as CK
from aprilslam_amd import _lib, localize, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE

pytestmark = pytest.mark.gpu

_runs = {}


def device(det, name):
    """(poses, result, covariance records) of asl_smooth_cov_batch on a case, run once"""
    if name not in _runs:
        obs, rec, seed, dist, sig, iters = VC.prior_only() if name == "prior_only" else VC.case(name)
        _runs[name] = det.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed, with_cov=True)
    return _runs[name]


@pytest.mark.parametrize("name", VC.DEVICE_CASES)
def test_device_matches_the_statement_at_its_own_poses(gpu_detector, name):
    obs, rec, seed, dist, sig, iters = VC.case(name)
    out, res, cov = device(gpu_detector, name)
    plain_out, plain_res = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=seed)
    assert out.tobytes() == plain_out.tobytes() and res.tobytes() == plain_res.tobytes()
    want = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig)[0]
    assert res["status"] == 0 and (want["status"] == 0).all()
    for k in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[k], want[k]), (name, k, cov[k], want[k])
    _, A = SV.dense_marginals(obs, rec, SC.K, dist, SC.TAG, out, *sig)
    worst = 0.0
    for f in range(len(out)):
        s = np.sqrt(np.diag(want["cov"][f]))
        worst = max(worst, float((np.abs(cov["cov"][f] - want["cov"][f]) / np.outer(s, s)).max()))
    print("%s: worst scaled covariance error %.3g" % (name, worst))
    for f in range(len(out)):
        CK.assert_cov_close(cov["cov"][f], want["cov"][f], A, (name, f))


@pytest.mark.parametrize("name", VC.NO_SOLVE_CASES + ["prior_only"])
def test_status_rules(gpu_detector, name):
    obs, rec, seed, dist, sig, iters = VC.prior_only() if name == "prior_only" else VC.case(name)
    out, res, cov = device(gpu_detector, name)
    want = SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, out, res, *sig)[0]
    status = 2 if name == "prior_only" else 1
    assert (want["status"] == status).all() and (res["status"] == 0) == (name == "prior_only")
    for k in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[k], want[k]), (name, k, cov[k], want[k])
    assert not cov["cov"].any() and cov["cov"].tobytes() == bytes(cov["cov"].nbytes)
    if name == "prior_only":
        assert (out["status"] == 6).all() and (cov["dof"] == -6).all()
    else:
        assert np.all(np.isin(out["status"], (1, 4))) and (cov["dof"] == 0).all()


def bar(name, out):
    """the comparison bar 600 eps kappa of a case at the device's poses"""
    obs, rec, seed, dist, sig, iters = VC.case(name)
    _, A = SV.dense_marginals(obs, rec, SC.K, dist, SC.TAG, out, *sig)
    return 600 * CK.EPS * SV.PC.scaled_condition(A)


def test_holes_structure_on_the_device(gpu_detector):
    out, res, cov = device(gpu_detector, "holes")
    std = SV.position_std(cov["cov"])
    rec, tol = VC.recorded(), bar("holes", out)
    print("holes position std", np.array2string(std, precision=5))
    for f, want in ((0, rec["holes_end_std"]), (6, rec["holes_end_std"]), (3, rec["holes_mid_std"])):
        assert abs(std[f] - want) <= VC.DIGITS + tol * want, (f, std[f], want)
    data = std[[1, 2, 4, 5]]
    assert rec["holes_data_std"][0] * (1 - tol) <= data.min() and data.max() <= rec["holes_data_std"][1] * (1 + tol)
    assert min(std[0], std[6]) > std[3] > data.max()


def test_hole70_structure_on_the_device(gpu_detector):
    out, res, cov = device(gpu_detector, "hole70")
    std = SV.position_std(cov["cov"])
    (peak, value), rims, tol = VC.recorded()["hole70_peak"], VC.recorded()["hole70_rims"], bar("hole70", out)
    assert int(np.argmax(std)) == peak and abs(std[peak] - value) <= VC.DIGITS + tol * value
    assert abs(std[1] - rims[0]) <= VC.DIGITS + tol * rims[0] and abs(std[72] - rims[1]) <= VC.DIGITS + tol * rims[1]
    assert np.all(np.diff(std[1:peak + 1]) > 0) and np.all(np.diff(std[peak:73]) < 0)


@pytest.fixture(scope="module")
def on_device(gpu_detector):
    """the 65-frame case on device buffers: localisation and smoothing with the covariance on one stream, no host wait"""
    import torch
    dev = torch.device("cuda:0")
    obs, rec, _, dist, sig, iters = VC.case("shape65_4_5")
    n, mt = obs.shape
    d_obs, d_map = CK.dev_bytes(obs, dev), CK.dev_bytes(rec, dev)
    d_seed = torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(_lib.SMOOTH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cov = torch.zeros(n * POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)

    def run():
        for t in (d_out, d_res, d_cov):
            t.zero_()
        torch.cuda.synchronize()
        gpu_detector.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), SC.K, dist, SC.TAG,
                                     stream=stream.cuda_stream)
        gpu_detector.smooth_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                   SC.K, dist, SC.TAG, *sig, max_iters=iters, stream=stream.cuda_stream, cov_ptr=d_cov.data_ptr())
        stream.synchronize()
        return tuple(t.cpu().numpy().tobytes() for t in (d_out, d_res, d_cov))
    return run, (d_obs, d_map, d_seed, d_out, d_res, d_cov, n, mt, len(rec), dist, sig)


def test_both_entry_points_agree_and_repeat_byte_for_byte(gpu_detector, on_device):
    run, _ = on_device
    first = run()
    obs, rec, _, dist, sig, iters = VC.case("shape65_4_5")
    out, res, cov = gpu_detector.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=None, with_cov=True)
    assert (out.tobytes(), res.tobytes(), cov.tobytes()) == first
    assert res["status"] == 0 and (cov["status"] == 0).all() and cov["cov"].any()
    assert run() == first


def test_refused_arguments_write_nothing(gpu_detector, on_device):
    import torch
    _, (d_obs, d_map, d_seed, d_out, d_res, d_cov, n, mt, n_ids, dist, sig) = on_device
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    Kc, dc = np.ascontiguousarray(SC.K), np.ascontiguousarray(dist)
    ok = [gpu_detector._h, d_obs.data_ptr(), n, mt, d_map.data_ptr(), n_ids, Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, SC.TAG,
          d_seed.data_ptr(), sig[0], sig[1], sig[2], 5, d_out.data_ptr(), d_res.data_ptr(), d_cov.data_ptr(), None]
    Knan = Kc.copy()
    Knan[0, 0] = np.nan
    nan, inf = float("nan"), float("inf")
    bad = [(1, None), (4, None), (6, None), (10, None), (15, None), (16, None), (2, 0), (2, 65536), (3, 0), (3, 257), (8, 3), (7, None),
           (6, Knan.ctypes.data_as(dp)), (9, nan), (9, inf), (11, 0.0), (11, nan), (12, -1.0), (12, inf), (13, 0.0), (13, nan), (14, 0), (14, 101),
           (15, d_seed.data_ptr()), (15, d_seed.data_ptr() + 160 * (n - 1)),
           (17, None), (17, d_out.data_ptr()), (17, d_out.data_ptr() + 160 * n - 8), (17, d_seed.data_ptr()), (17, d_seed.data_ptr() + 160 * n - 8)]
    for t in (d_out, d_res, d_cov):
        t.fill_(0xAB)
    seed_before = d_seed.cpu().numpy().tobytes()
    torch.cuda.synchronize()
    for k, v in bad:
        a = list(ok)
        a[k] = v
        assert L.asl_smooth_cov_frames_device(*a) == -1, (k, v)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == 0xAB).all() for t in (d_out, d_res, d_cov)) and d_seed.cpu().numpy().tobytes() == seed_before
    assert L.asl_smooth_cov_frames_device(*ok) == 0
    torch.cuda.synchronize()
    assert not (d_res.cpu().numpy() == 0xAB).all() and (d_cov.cpu().numpy().view(POSE_COV_DTYPE)["status"] == 0).all()
    # the host form refuses the same way
    obs, rec = VC.case("shape65_4_5")[:2]
    out = np.full(n * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    res = np.full(64, 0xAB, dtype=np.uint8)
    cov = np.full(n * POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    hk = [gpu_detector._h, obs.ctypes.data, n, mt, rec.ctypes.data, n_ids, Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, SC.TAG, None,
          sig[0], sig[1], sig[2], 5, out.ctypes.data, res.ctypes.data, cov.ctypes.data]
    for k, v in ((1, None), (4, None), (6, None), (15, None), (16, None), (17, None), (2, 0), (3, 257), (8, 2), (11, -1.0), (13, nan), (14, 0)):
        a = list(hk)
        a[k] = v
        assert L.asl_smooth_cov_batch(*a) == -1, (k, v)
    assert (out == 0xAB).all() and (res == 0xAB).all() and (cov == 0xAB).all()


def test_tag_detector_and_slam_surface():
    """the four-frame sequence of test_gpu_smooth's surface test (three rendered frames around a blank one) with with_cov"""
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.tag_detector import TagDetector
    from aprilslam_amd.localize import TagMap
    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, id_limit=0)
    cams = LC.trajectory(520)[:3]
    frames = [synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r)[0] for p, r in cams]
    frames.insert(2, np.zeros_like(frames[0]))
    d, p, npf = td.detector._det.detect_host(np.stack(frames), K=SC.K, dist=np.zeros(4), tag_size=SC.TAG)

    class _Log:
        def info(self, m):
            pass
    slam = SLAM(_Log(), {"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, detector=td)
    for det in slam.detect(frames[0]):
        slam.get_pose(det)
    kw = dict(sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2)
    first = td.localize_sequence(d, p, npf, tm, with_cov=True, **kw)
    assert first.poses["status"].tolist() == [0, 0, 6, 0]
    for r in (first, slam.localize_sequence(d, p, npf, with_cov=True, **kw)):
        assert r.ok and r.cov.shape == (4, 6, 6) and r.cov_status.tolist() == [0, 0, 0, 0]
        pos = np.linalg.norm(r.pose_std()[1], axis=1)
        assert pos[2] > pos[1] and pos[2] > pos[3], pos
        for a, b in zip(r.pose_std(), localize.pose_std(r.cov)):
            assert np.array_equal(a, b)
    plain = td.localize_sequence(d, p, npf, tm, **kw)
    assert plain.poses.tobytes() == first.poses.tobytes() and plain.result.tobytes() == first.result.tobytes()
    with pytest.raises(ValueError):
        plain.cov
    with pytest.raises(ValueError):
        plain.cov_status
