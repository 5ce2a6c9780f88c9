"""Camera calibration on the device (asl_calibrate_frames_device / asl_calibrate_batch, k_calib.inc) against the NumPy
statement (tests/calib_ref.py) and against the renderer's ground truth."""
import numpy as np
import pytest

import calib_cases as CC
import calib_ref as CR
import localize_cases as LC
from aprilslam_amd import _lib, synth
from aprilslam_amd.calibrate import CALIB_RESULT_DTYPE, CalibrationResult
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max())) if b.size else 0.0


def assert_same(got, want, tol):
    (gr, gp), (wr, wp) = got, want
    assert gr["status"] == wr["status"] and gr["n_frames_used"] == wr["n_frames_used"] and gr["n_corners"] == wr["n_corners"]
    assert np.array_equal(gp["status"], wp["status"]) and np.array_equal(gp["n_tags"], wp["n_tags"])
    assert rel(gr["K"], wr["K"]) <= tol, (gr["K"], wr["K"])
    assert np.abs(gr["dist"] - wr["dist"]).max() <= tol * max(1.0, np.abs(wr["dist"]).max())
    assert np.array_equal(gr["std"] == 0, wr["std"] == 0)
    assert rel(gr["std"], wr["std"]) <= max(tol, 1e-7), (gr["std"], wr["std"])   # a ratio of small sums: a few digits fewer
    for g, w in zip(gp, wp):
        assert LC.rel_err(g["T"], w["T"]) <= tol
    assert abs(gr["rms_px"] - wr["rms_px"]) <= 1e-6 * max(1.0, wr["rms_px"])
    assert abs(gr["rms_init_px"] - wr["rms_init_px"]) <= 1e-6 * max(1.0, wr["rms_init_px"])


@pytest.mark.parametrize("case", [c[0] for c in CC.cpu_cases()])
def test_kernel_matches_the_statement_on_the_cpu_cases(gpu_detector, case):
    name, obs, rec, kw = [c for c in CC.cpu_cases() if c[0] == case][0]
    got = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    want = CR.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    assert_same(got, want, 1e-9)


def webcam_cameras(n, seed=11):
    rng = np.random.default_rng(seed)
    tags = synth.random_scene(CC.WEBCAM_W, CC.WEBCAM_H, 12, rng, fov_y_deg=CC.WEBCAM_FOV)
    return tags, [(tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-4, 4, 3))) for _ in range(n)]


@pytest.fixture(scope="module")
def webcam_block():
    """128 frames of the distorted webcam rendered on the device -> detect -> asl_obs records -> calibrate, one stream, one
    read-back at the end"""
    import torch
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n, max_tags, w, h = 128, 16, CC.WEBCAM_W, CC.WEBCAM_H
    tags, cams = webcam_cameras(n)
    planes, _ = synth.render_planes(w, h, tags, LC.TAG_OUTER, cams, fov_y_deg=CC.WEBCAM_FOV, dist=CC.WEBCAM_DIST)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    K = synth.camera_matrix(w, h, CC.WEBCAM_FOV)
    rec = TagMap.from_scene(tags).as_records()
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_tex = torch.from_numpy(tex).to(dev)
    d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty(CALIB_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_poses = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    det.render_frames_device(frames.data_ptr(), n, w, h, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2], tex.shape[1],
                             0.5 * LC.TAG_OUTER, K=K, dist=CC.WEBCAM_DIST, stream=st)
    det.submit_device(frames.data_ptr(), n, 3, w, h, stream=st)
    det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=st)
    det.calibrate_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), len(rec), LC.TAG_INNER, w, h, d_res.data_ptr(), d_poses.data_ptr(),
                         n_dist=5, stream=st)
    stream.synchronize()
    res = d_res.cpu().numpy().view(CALIB_RESULT_DTYPE)[0]
    poses = d_poses.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, max_tags)
    det.collect()
    yield det, obs, rec, res, poses, cams, K, (d_obs, d_map, d_res, d_poses)
    det.close()


def test_device_chain_matches_the_statement_and_the_truth(webcam_block):
    _, obs, rec, res, poses, cams, K, _ = webcam_block
    want = CR.calibrate(obs, rec, LC.TAG_INNER, CC.WEBCAM_W, CC.WEBCAM_H, n_dist=5)
    # detector corners: a trial accepted by one side and rejected by the other at the rounding level changes the LM path
    assert_same((res, poses), want, 1e-7)
    assert res["status"] == 0 and res["n_frames_used"] >= 120
    e = np.abs(res["K"] - K)
    assert e[0, 0] / K[0, 0] <= 2e-3 and e[1, 1] / K[1, 1] <= 2e-3 and e[0, 2] <= 1.5 and e[1, 2] <= 1.5, res["K"]
    assert CC.field_err(res["K"], res["dist"], K, CC.WEBCAM_DIST, CC.WEBCAM_W, CC.WEBCAM_H) <= 0.5
    assert res["rms_px"] < 0.3 and (res["std"][:9] > 0).all()
    rot = [LC.rot_err(p["T"], LC.world_from_camera(*c)) for p, c in zip(poses, cams) if p["status"] == 0]
    assert len(rot) == res["n_frames_used"] and max(rot) <= 3e-3


def test_repeated_calls_give_identical_bytes(webcam_block):
    import torch
    det, obs, rec, res, poses, _, _, (d_obs, d_map, d_res, d_poses) = webcam_block
    n, max_tags = obs.shape
    for _ in range(2):
        d_res.zero_()
        d_poses.zero_()
        det.calibrate_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), len(rec), LC.TAG_INNER, CC.WEBCAM_W, CC.WEBCAM_H,
                             d_res.data_ptr(), d_poses.data_ptr(), n_dist=5, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d_res.cpu().numpy().tobytes() == res.tobytes()
        assert d_poses.cpu().numpy().tobytes() == poses.tobytes()


def test_principal_point_of_an_off_centre_window():
    """bench frames (1280x720, the pinhole of fov 45) detected through a window at (x0, y0): a pointer offset with the full
    row stride.  The principal point is the true one in window coordinates, not the window's centre."""
    import torch

    import bench
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        n, max_tags = 64, 32
        frames, _, _ = bench.render_stream_device(det, n, dev)
        x0, y0, w, h = 240, 100, 960, 560
        st = torch.cuda.current_stream(dev).cuda_stream
        offset = (y0 * LC.W + x0) * 3
        det.submit_device(frames.data_ptr() + offset, n, 3, w, h, stride=LC.W * 3, frame_pitch=LC.W * LC.H * 3, stream=st)
        d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=st)
        torch.cuda.synchronize(dev)
        det.collect()
        obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, max_tags)
        rec = TagMap.from_scene(LC.bench_scene()).as_records()
        res, poses = det.calibrate(obs, rec, LC.TAG_INNER, w, h, n_dist=0)
        K = synth.camera_matrix(LC.W, LC.H, 45.0)
        assert res["status"] == 0 and res["n_frames_used"] >= 60
        assert abs(res["K"][0, 2] - (K[0, 2] - x0)) <= 1.5 and abs(res["K"][1, 2] - (K[1, 2] - y0)) <= 1.5, res["K"]
        assert abs(res["K"][0, 0] / K[0, 0] - 1) <= 2e-3 and abs(res["K"][1, 1] / K[1, 1] - 1) <= 2e-3
        assert_same((res, poses), CR.calibrate(obs, rec, LC.TAG_INNER, w, h, n_dist=0), 1e-7)
    finally:
        det.close()


def test_tag_detector_calibrate_and_camera_params():
    from aprilslam_amd.tag_detector import TagDetector
    tags, cams = webcam_cameras(12)
    frames = [synth.render_frame(CC.WEBCAM_W, CC.WEBCAM_H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r,
                                 fov_y_deg=CC.WEBCAM_FOV, dist=CC.WEBCAM_DIST)[0] for p, r in cams]
    td = TagDetector({"camera_matrix": np.eye(3), "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER, id_limit=0)
    cr = td.calibrate(frames, TagMap.from_scene(tags), n_dist=5)
    assert isinstance(cr, CalibrationResult) and cr.ok and cr.n_frames_used == len(frames)
    K = synth.camera_matrix(CC.WEBCAM_W, CC.WEBCAM_H, CC.WEBCAM_FOV)
    assert abs(cr.K[0, 0] / K[0, 0] - 1) <= 3e-3 and abs(cr.K[0, 2] - K[0, 2]) <= 2.0
    td2 = TagDetector(cr.camera_params, tag_size=LC.TAG_INNER, id_limit=0)
    r = td2.localize(td2.detect(frames[0]), TagMap.from_scene(tags))
    assert r["ok"] and LC.rot_err(r["T"], LC.world_from_camera(*cams[0])) <= 3e-3


def test_errors_and_record_size(gpu_detector):
    import torch
    assert CALIB_RESULT_DTYPE.itemsize == 216
    dev = torch.device("cuda:0")
    obs, rec, _ = CC.scene_case(n=4)
    d_obs = torch.from_numpy(obs.view(np.uint8).copy()).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_res = torch.zeros(CALIB_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_poses = torch.zeros((4, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    ok = dict(obs_ptr=d_obs.data_ptr(), n_frames=4, max_tags=obs.shape[1], map_ptr=d_map.data_ptr(), n_ids=len(rec), tag_size=LC.TAG_INNER,
              width=CC.W, height=CC.H, result_ptr=d_res.data_ptr(), poses_ptr=d_poses.data_ptr(), n_dist=5, flags=0, max_iters=5)
    gpu_detector.calibrate_device(**ok)
    torch.cuda.synchronize()
    assert d_res.cpu().numpy().view(CALIB_RESULT_DTYPE)[0]["status"] == 0
    bad = [dict(obs_ptr=0), dict(map_ptr=0), dict(result_ptr=0), dict(poses_ptr=0), dict(max_tags=0), dict(max_tags=257), dict(n_ids=0),
           dict(tag_size=0.0), dict(tag_size=-1.0), dict(width=0), dict(height=-3), dict(max_iters=0), dict(n_frames=0), dict(flags=8)]
    for b in bad:
        with pytest.raises(_lib.AslError):
            gpu_detector.calibrate_device(**{**ok, **b})
    with pytest.raises(ValueError):
        gpu_detector.calibrate_device(**{**ok, "n_dist": 3})
    L = _lib.load()
    res = np.zeros((), dtype=CALIB_RESULT_DTYPE)
    poses = np.zeros(4, dtype=CAM_POSE_DTYPE)
    args = [gpu_detector._h, obs.ctypes.data, 4, obs.shape[1], rec.ctypes.data, len(rec), LC.TAG_INNER, CC.W, CC.H, None, 5, 0, 5,
            res.ctypes.data, poses.ctypes.data]
    assert L.asl_calibrate_batch(*args) == 0 and res["status"] == 0
    for k, v in ((1, None), (4, None), (13, None), (14, None), (10, 3), (10, 1), (3, 300), (12, 0), (6, 0.0)):
        a = list(args)
        a[k] = v
        assert L.asl_calibrate_batch(*a) == -1, (k, v)
    assert L.asl_calibrate_batch(None, *args[1:]) == -1
