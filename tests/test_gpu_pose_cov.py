"""Pose covariance on the device (asl_localize_cov_frames_device / asl_localize_cov_batch in k_localize.inc,
asl_pose_cov_device / asl_solve_pnp_cov_batch in k_posecov.inc) against the NumPy statement (localize_ref.pose_cov over
tests/pose_cov_ref.py), to the covariance bar of solver_checks.assert_cov_close."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import solver_edge_cases as SE
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap, pose_std
from solver_checks import assert_cov_close

pytestmark = pytest.mark.gpu

K = synth.camera_matrix(LC.W, LC.H, 45.0)
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
SIGMA = 0.5            # the given sigma of the comparisons
NOISE = 0.2            # corner noise (px) of the copies the estimated sigma is compared on
BENCH_RECORDS = 20480  # bench.py: 1024 frames x 20 tags
PNP_SIZES = (1, 3, 4, 5, 63, 64, 65, 1000, BENCH_RECORDS)


def loc_cases():
    """(name, obs, map records, dist, gate): localize_cases.cpu_cases and solver_edge_cases.loc_cases"""
    return list(LC.cpu_cases(K)) + [c[:5] for c in SE.loc_cases()]


LOC_NAMES = [c[0] for c in loc_cases()]


def loc_case(name):
    return [c for c in loc_cases() if c[0] == name][0]


def noisy(obs, seed):
    out = obs.copy()
    rng = np.random.default_rng(seed)
    out["corners"] = (obs["corners"].astype(np.float64) + rng.normal(scale=NOISE, size=obs["corners"].shape)).astype(np.float32)
    return out


def check_localize_cov(obs, rec, dist, gate, sigma_px, out, cov, compare_cov):
    """device records against the statement evaluated at the device's own pose on the statement's active set"""
    traces = []
    want = LR.localize(obs, rec, K, dist, LC.TAG_INNER, gate, traces=traces)
    one = LR.OneCamera(LR.camera(K, dist))
    for f, (g, w, c) in enumerate(zip(out, want, cov)):
        assert g["status"] == w["status"] and g["n_rejected"] == w["n_rejected"] and g["n_tags"] == w["n_tags"], f
        if g["status"] != 0:
            assert c["status"] == 1 and c["dof"] == 0 and c["sigma_px"] == sigma_px and not c["cov"].any(), f
            continue
        Xw, uv, ci = LR.frame_points(one, obs[f], rec, LC.TAG_INNER, traces[f]["active"])
        R = g["T"][:3, :3].T
        t = -(R @ g["T"][:3, 3])
        ref, sig, dof, status = LR.pose_cov(one, R, t, Xw, uv, ci, sigma_px)
        assert status == 0 and c["status"] == 0 and c["dof"] == dof == 8 * g["n_tags"] - 6, f
        assert abs(c["sigma_px"] - sig) <= 1e-6 * sig, (f, c["sigma_px"], sig)
        if compare_cov:
            assert_cov_close(c["cov"], ref, one.linearise(R, t, Xw, uv, ci)[1], f)


@pytest.mark.parametrize("case", LOC_NAMES)
def test_localize_cov_matches_the_statement(gpu_detector, case):
    """given sigma on the case as it is (exact corners: a cost at rounding level has no sigma to estimate)"""
    name, obs, rec, dist, gate = loc_case(case)
    plain = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    out, cov = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate, sigma_px=SIGMA)
    assert out.tobytes() == plain.tobytes()
    check_localize_cov(obs, rec, dist, gate, SIGMA, out, cov, True)


@pytest.mark.parametrize("case", LOC_NAMES)
def test_localize_cov_estimated_sigma(gpu_detector, case):
    """sigma_px = 0 on a copy of the case with fixed-seed corner noise: sigma to 1e-6 relative, and the same pose bytes"""
    name, obs, rec, dist, gate = loc_case(case)
    obs = noisy(obs, 11)
    plain = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    out, cov = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate, sigma_px=0.0)
    assert out.tobytes() == plain.tobytes()
    check_localize_cov(obs, rec, dist, gate, 0.0, out, cov, True)
    ok = out["status"] == 0
    assert (cov["sigma_px"][ok] > 0).all()


@pytest.mark.parametrize("case", LOC_NAMES)
def test_localize_cov_device_form_and_determinism(gpu_detector, case):
    """the device-pointer form: d_out the bytes of asl_localize_batch, d_cov the bytes of the host form, twice"""
    import torch
    name, obs, rec, dist, gate = loc_case(case)
    dev = torch.device("cuda:0")
    n, mt = obs.shape
    plain = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    out, cov = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate, sigma_px=SIGMA)
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(-1)).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    for _ in range(2):
        d_out = torch.full((n * CAM_POSE_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
        d_cov = torch.full((n * _lib.POSE_COV_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
        gpu_detector.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, dist, LC.TAG_INNER,
                                     max_tag_rms_px=gate, stream=torch.cuda.current_stream().cuda_stream, cov_ptr=d_cov.data_ptr(),
                                     sigma_px=SIGMA)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == plain.tobytes()
        assert d_cov.cpu().numpy().tobytes() == cov.tobytes()


# ---- per-tag PnP

def pnp_records(n, dist, seed):
    """n tags of side TAG_INNER at 30..90 units, tilted 15..55 degrees, corners with NOISE px of noise (float32)"""
    rng = np.random.default_rng(seed)
    cam = LR.camera(K, dist)
    obj = np.c_[LR.object_corners(LC.TAG_INNER), np.zeros(4)]
    c = np.zeros((n, 4, 2), dtype=np.float32)
    for i in range(n):
        ax = rng.normal(size=3)
        R = LR.rodrigues(ax / np.linalg.norm(ax) * np.radians(rng.uniform(15, 55))) @ np.diag([1.0, -1.0, -1.0])
        z = rng.uniform(30, 90)
        t = np.array([rng.uniform(-0.3, 0.3) * z, rng.uniform(-0.2, 0.2) * z, z])
        c[i] = LR.project(cam, obj @ R.T + t) + rng.normal(scale=NOISE, size=(4, 2))
    return c


def check_pnp_cov(corners, T, posed, dist, sigma_px, cov, compare_cov):
    cam = LR.camera(K, dist)
    for i, c in enumerate(cov):
        if not posed[i]:
            assert c["status"] == 1 and c["dof"] == 0 and c["sigma_px"] == sigma_px and not c["cov"].any(), i
            continue
        Xw, uv = LR.tag_points(corners[i].reshape(8), LC.TAG_INNER)
        R, t = T[i][:3, :3], T[i][:3, 3]
        ref, sig, dof, status = LR.pose_cov(LR.OneCamera(cam), R, t, Xw, uv, None, sigma_px, False)
        assert status == 0 and c["status"] == 0 and c["dof"] == dof == 2, i
        assert abs(c["sigma_px"] - sig) <= 1e-6 * sig, (i, c["sigma_px"], sig)
        if compare_cov:
            assert_cov_close(c["cov"], ref, LR.linearise(cam, R, t, Xw, uv)[1], i)


@pytest.mark.parametrize("nd", [0, 5])
@pytest.mark.parametrize("n", PNP_SIZES)
def test_pnp_cov_matches_the_statement(gpu_detector, n, nd):
    """host form on solve_pnp's own output and the device form on asl_obs records, every third record without flags & 2;
    given sigma for the covariance, sigma_px = 0 for the estimate; the same bytes from both forms and on a second run"""
    import torch
    dist = DIST5 if nd else None
    corners = pnp_records(n, dist, 1000 + n + nd)
    _, _, T, ok = gpu_detector.solve_pnp(corners, K, dist, LC.TAG_INNER)
    assert ok.all()
    posed = np.arange(n) % 3 != 1
    Th = np.where(posed[:, None, None], T, np.nan)            # the host form: a pose that is not finite is no pose
    rec = np.zeros(n, dtype=_lib.OBS_DTYPE)
    rec["id"] = np.arange(n) % 7
    rec["flags"] = np.where(posed, 3, 1)
    rec["corners"] = corners.reshape(n, 8)
    rec["T"] = T.reshape(n, 16)[:, :12]
    dev = torch.device("cuda:0")
    d_obs = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)
    for sigma_px in (SIGMA, 0.0):
        cov = gpu_detector.pose_cov(corners, Th, K, dist, LC.TAG_INNER, sigma_px)
        check_pnp_cov(corners, T, posed, dist, sigma_px, cov, sigma_px > 0)   # the estimate: sigma alone, it only scales the same matrix
        for _ in range(2):
            d_cov = torch.full((n * _lib.POSE_COV_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
            gpu_detector.pose_cov_device(d_obs.data_ptr(), n, d_cov.data_ptr(), K, dist, LC.TAG_INNER, sigma_px,
                                         stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert d_cov.cpu().numpy().tobytes() == cov.tobytes()
        assert gpu_detector.pose_cov(corners, Th, K, dist, LC.TAG_INNER, sigma_px).tobytes() == cov.tobytes()


# ---- the ABI

def test_bad_sigma_is_rejected_and_nothing_is_written(gpu_detector):
    import torch
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    Kc = np.ascontiguousarray(K)
    name, obs, rec, dist, gate = loc_case("exact")
    obs = np.ascontiguousarray(obs)
    n, mt = obs.shape
    dev = torch.device("cuda:0")
    d_obs = torch.from_numpy(obs.view(np.uint8).reshape(-1)).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    corners = pnp_records(5, None, 3)
    _, _, T, _ = gpu_detector.solve_pnp(corners, K, None, LC.TAG_INNER)
    T = np.ascontiguousarray(T)
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        out = np.full(n, 0x55, dtype=np.uint8).repeat(CAM_POSE_DTYPE.itemsize)
        cov = np.full(n * _lib.POSE_COV_DTYPE.itemsize, 0x55, dtype=np.uint8)
        assert L.asl_localize_cov_batch(gpu_detector._h, obs.ctypes.data, n, mt, rec.ctypes.data, len(rec), Kc.ctypes.data_as(dp), None, 0,
                                        LC.TAG_INNER, 0.0, bad, out.ctypes.data, cov.ctypes.data) == -1, bad
        assert (out == 0x55).all() and (cov == 0x55).all()
        d_out = torch.full((n * CAM_POSE_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device=dev)
        d_cov = torch.full((n * _lib.POSE_COV_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device=dev)
        assert L.asl_localize_cov_frames_device(gpu_detector._h, d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), Kc.ctypes.data_as(dp),
                                                None, 0, LC.TAG_INNER, 0.0, bad, d_out.data_ptr(), d_cov.data_ptr(), None) == -1, bad
        assert L.asl_pose_cov_device(gpu_detector._h, d_obs.data_ptr(), n * mt, Kc.ctypes.data_as(dp), None, 0, LC.TAG_INNER, bad,
                                     d_cov.data_ptr(), None) == -1, bad
        torch.cuda.synchronize()
        assert bool((d_out == 0x55).all()) and bool((d_cov == 0x55).all())
        pc = np.full(5 * _lib.POSE_COV_DTYPE.itemsize, 0x55, dtype=np.uint8)
        assert L.asl_solve_pnp_cov_batch(gpu_detector._h, corners.ctypes.data_as(C.POINTER(C.c_float)), T.ctypes.data_as(dp),
                                         Kc.ctypes.data_as(dp), None, 0, LC.TAG_INNER, bad, pc.ctypes.data, 5) == -1, bad
        assert (pc == 0x55).all()
        with pytest.raises(_lib.AslError):
            gpu_detector.localize(obs, rec, K, None, LC.TAG_INNER, sigma_px=bad)
    with pytest.raises(_lib.AslError):        # a covariance call without room for the covariance
        gpu_detector.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_obs.data_ptr(), K, None, LC.TAG_INNER, cov_ptr=0)


def test_record_layout():
    """asl_pose_cov is 304 bytes and POSE_COV_DTYPE has the C layout (test_abi.py's check for the other records)"""
    dt = _lib.POSE_COV_DTYPE
    assert dt.itemsize == 36 * 8 + 8 + 4 + 4 == 304
    c = np.dtype(dt.descr, align=True)
    assert c.itemsize == dt.itemsize and [c.fields[f][1] for f in c.names] == [dt.fields[f][1] for f in dt.names]
    assert [dt.fields[f][1] for f in ("cov", "sigma_px", "dof", "status")] == [0, 288, 296, 300]
    for name in ("asl_localize_cov_frames_device", "asl_localize_cov_batch", "asl_pose_cov_device", "asl_solve_pnp_cov_batch"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)


def test_tag_detector_and_slam_surface():
    """one rendered frame through TagDetector.localize(with_cov=True), localize_batch, get_poses_cov and SLAM.localize"""
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.tag_detector import TagDetector
    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": K, "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER, id_limit=0)
    pos, rot = LC.trajectory(16)[3]
    frame, _ = synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=pos, cam_rotation_deg=rot)
    dets = td.detect(frame)
    plain = td.localize(dets, tm)
    assert sorted(plain) == ["T", "n_rejected", "n_tags", "ok", "rms_px", "status"]
    r = td.localize(dets, tm, with_cov=True)
    assert sorted(r) == sorted(list(plain) + ["cov", "sigma_px", "cov_status"])
    assert r["ok"] and r["cov_status"] == 0 and np.array_equal(r["T"], plain["T"])
    cov = r["cov"]
    assert cov.shape == (6, 6) and np.array_equal(cov, cov.T) and (np.diag(cov) > 0).all() and r["sigma_px"] > 0
    rot_std, tr_std = pose_std(cov)
    assert rot_std.shape == (3,) and tr_std.shape == (3,) and np.allclose(np.r_[rot_std, tr_std] ** 2, np.diag(cov))
    given = td.localize(dets, tm, with_cov=True, sigma_px=0.25)
    assert given["sigma_px"] == 0.25
    assert np.allclose(given["cov"] / 0.25 ** 2, cov / r["sigma_px"] ** 2, rtol=1e-9, atol=0)

    d, p, npf = td.detector._det.detect_host(np.stack([frame, frame]), K=K, dist=np.zeros(4), tag_size=LC.TAG_INNER)
    rb = td.localize_batch(d, p, npf, tm)
    assert rb.dtype == CAM_POSE_DTYPE and len(rb) == 2
    rb2, cb = td.localize_batch(d, p, npf, tm, with_cov=True)
    assert rb2.tobytes() == rb.tobytes() and cb.dtype == _lib.POSE_COV_DTYPE and len(cb) == 2 and (cb["status"] == 0).all()
    assert np.allclose(cb["cov"][1], cov, rtol=1e-6, atol=0)

    ok, rvec, tvec, T, pc = td.get_poses_cov(dets, 0.3)
    ok0, rvec0, tvec0, T0 = td.get_poses(dets)
    assert np.array_equal(ok, ok0) and np.array_equal(T, T0) and np.array_equal(rvec, rvec0) and np.array_equal(tvec, tvec0)
    assert pc.shape == (len(dets),) and pc["cov"].shape == (len(dets), 6, 6)
    assert (pc["status"][ok] == 0).all() and (pc["status"][~ok] == 1).all() and (pc["sigma_px"][ok] == 0.3).all()
    for c in pc["cov"][ok]:
        assert np.array_equal(c, c.T) and (np.diag(c) > 0).all()
    # one tag determines the pose far worse than all of them together: the spread DESIGN 7b reports, now in the output
    assert np.median(pose_std(pc["cov"][ok])[0]) > 10 * np.median(pose_std(given["cov"] * (0.3 / 0.25) ** 2)[0])
    assert td.get_poses_cov([], 0.3)[4].shape == (0,)

    class _Log:
        def info(self, m):
            pass
    slam = SLAM(_Log(), {"camera_matrix": K, "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER, detector=td)
    dets = slam.detect(frame)
    for det in dets:
        slam.get_pose(det)
    res = slam.localize(dets)
    assert "cov" not in res
    res = slam.localize(dets, with_cov=True, sigma_px=0.3)
    assert res["ok"] and res["cov"].shape == (6, 6) and res["sigma_px"] == 0.3
