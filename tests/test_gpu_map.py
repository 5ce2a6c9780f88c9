"""Tag-map reconstruction on the device (asl_map_frames_device / asl_map_batch, k_map.inc) against the NumPy statement
(tests/map_ref.py), on a device-rendered stream end to end (detect -> pack -> map -> localise on one stream), determinism
and argument errors."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as CC
import localize_cases as LC
import map_cases as MC
import map_ref as MR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE

pytestmark = pytest.mark.gpu

K = MC.K_bench()


def assert_same(got, want, tol):
    gr, gm, gs, gp = got
    wr, wm, ws, wp = want
    for k in ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "world_id", "status"):
        assert gr[k] == wr[k], (k, gr[k], wr[k])
    assert abs(gr["rms_px"] - wr["rms_px"]) <= 1e-6 * max(1.0, wr["rms_px"])
    assert abs(gr["rms_seed_px"] - wr["rms_seed_px"]) <= 1e-6 * max(1.0, wr["rms_seed_px"])
    assert np.array_equal(gm["valid"], wm["valid"])
    for i in np.flatnonzero(wm["valid"]):
        assert LC.rel_err(MR.rec4(gm["T"][i]), MR.rec4(wm["T"][i])) <= tol, (i, LC.rel_err(MR.rec4(gm["T"][i]), MR.rec4(wm["T"][i])))
    assert np.array_equal(gp["status"], wp["status"]) and np.array_equal(gp["n_tags"], wp["n_tags"])
    assert np.array_equal(gp["n_rejected"], wp["n_rejected"]) and np.array_equal(gp["seed_slot"], wp["seed_slot"])
    for f in np.flatnonzero(wp["status"] == 0):
        assert LC.rel_err(gp["T"][f], wp["T"][f]) <= tol, (f, LC.rel_err(gp["T"][f], wp["T"][f]))
    if gs is not None and ws is not None:
        np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("case", [c[0] for c in MC.cpu_cases(K)])
def test_kernel_matches_the_statement_on_the_cpu_cases(gpu_detector, case):
    name, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == case][0]
    got = gpu_detector.build_map(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w)
    want = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w)[:4]
    assert_same(got, want, 1e-9)


def test_the_same_input_gives_the_same_bytes(gpu_detector):
    obs, _, _ = MC.exact_block(12, dist=MC.DIST5, K=K)
    a = gpu_detector.build_map(obs, MC.N_IDS, K, MC.DIST5, LC.TAG_INNER)
    b = gpu_detector.build_map(obs, MC.N_IDS, K, MC.DIST5, LC.TAG_INNER)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    empty = np.zeros((5, obs.shape[1]), dtype=_lib.OBS_DTYPE)
    empty["id"] = -1
    c = gpu_detector.build_map(np.concatenate([obs, empty]), MC.N_IDS, K, MC.DIST5, LC.TAG_INNER)
    assert a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes() and a[3].tobytes() == c[3][:12].tobytes()


def test_argument_errors_fail_loudly(gpu_detector):
    obs, _, _ = MC.exact_block(4, K=K)
    with pytest.raises(ValueError):
        gpu_detector.build_map(obs, MC.N_IDS, K, np.zeros(3), LC.TAG_INNER)
    L, h = gpu_detector._L, gpu_detector._h
    dp = C.POINTER(C.c_double)
    Kc = np.ascontiguousarray(K)
    res = np.zeros((), dtype=_lib.MAP_RESULT_DTYPE)
    tm = np.zeros(MC.N_IDS, dtype=_lib.MAP_TAG_DTYPE)
    poses = np.zeros(4, dtype=CAM_POSE_DTYPE)
    o = np.ascontiguousarray(obs)

    def call(obs_p=o.ctypes.data, mt=obs.shape[1], nd=0, dist=None, map_p=tm.ctypes.data, world=-1, n_ids=MC.N_IDS, nf=4):
        return L.asl_map_batch(h, obs_p, nf, mt, n_ids, Kc.ctypes.data_as(dp), dist, nd, LC.TAG_INNER, world, 30, map_p, None,
                               poses.ctypes.data, res.ctypes.data)
    assert call() == 0
    assert call(nd=3) != 0
    assert call(mt=0) != 0 and call(mt=257) != 0
    assert call(obs_p=None) != 0 and call(map_p=None) != 0
    assert call(nd=4, dist=None) != 0
    missing = next(i for i in range(MC.N_IDS) if i not in set(obs["id"].ravel()))
    assert call(world=missing) != 0 and b"not seen" in L.asl_last_error()
    # 1001 frames, each with ids (k, k + 1): 1002 tags
    big = np.zeros((1001, 2), dtype=_lib.OBS_DTYPE)
    big["id"][:, 0] = np.arange(1001)
    big["id"][:, 1] = np.arange(1001) + 1
    big["flags"] = 3
    big["T"][..., 11] = 100.0
    big["T"][..., 0] = big["T"][..., 5] = big["T"][..., 10] = 1.0
    with pytest.raises(_lib.AslError, match="1000"):
        gpu_detector.build_map(big, 1002, K, None, LC.TAG_INNER)


@pytest.fixture(scope="module")
def device_chain():
    """128 bench frames rendered on the device -> detect + PnP -> asl_obs -> map -> localisation against the map, one stream,
    read back at the end"""
    import torch

    import bench
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n, max_tags, n_ids = 128, 32, 64
    Kr = synth.camera_matrix(LC.W, LC.H, 45.0)
    frames, _, _ = bench.render_stream_device(det, n, dev)
    stream = torch.cuda.Stream(dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), **u8)
    d_map = torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), **u8)
    d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty((n, CAM_POSE_DTYPE.itemsize), **u8)
    d_res = torch.empty((_lib.MAP_RESULT_DTYPE.itemsize,), **u8)
    d_loc = torch.empty((n, CAM_POSE_DTYPE.itemsize), **u8)
    det.submit_device(frames.data_ptr(), n, 3, LC.W, LC.H, stream=stream.cuda_stream, K=Kr, dist=np.zeros(4), tag_size=LC.TAG_INNER)
    det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=stream.cuda_stream)
    det.build_map_device(d_obs.data_ptr(), n, max_tags, n_ids, Kr, None, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(),
                         d_poses.data_ptr(), d_res.data_ptr(), stream=stream.cuda_stream)
    det.localize_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), n_ids, d_loc.data_ptr(), Kr, None, LC.TAG_INNER,
                        stream=stream.cuda_stream)
    stream.synchronize()
    got = (d_res.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(()), d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(n_ids),
           d_std.cpu().numpy(), d_poses.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n))
    loc = d_loc.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, max_tags)
    det.collect()
    yield det, Kr, obs, got, loc, bench.camera_trajectory(n)
    det.close()


def test_device_chain_matches_the_statement_and_the_truth(device_chain):
    _, Kr, obs, got, loc, traj = device_chain
    want = MR.map_frames(obs, 64, Kr, None, LC.TAG_INNER)[:4]
    assert_same(got, want, 1e-7)
    res, tmap, _, poses = got
    assert res["status"] == 0 and res["rms_px"] < 0.5 and res["n_frames_used"] >= 120
    tags = LC.bench_scene()
    et, er, ec = MC.map_errors(tmap, poses, tags, traj, int(res["world_id"]))
    assert et < 0.05 * LC.TAG_INNER and er < 0.01, (et, er)
    # the host path it replaces (map_init seeding + the pinhole LM) on the same read-back block: no better than the device
    world, ids, cam_idx, cam_T, tag_T, _ = MC.host_path(obs, Kr, LC.TAG_INNER, 60)
    hm, hp = MC.host_records(64, len(obs), ids, cam_idx, cam_T, tag_T)
    ht, hr, hc = MC.map_errors(hm, hp, tags, traj, world)
    assert world == res["world_id"]
    assert et <= ht * (1 + 1e-6) + 1e-9 and er <= hr * (1 + 1e-6) + 1e-9 and ec <= hc * (1 + 1e-6) + 1e-9, ((et, er, ec), (ht, hr, hc))


def test_localisation_against_the_surveyed_map_gives_the_map_poses(device_chain):
    _, _, _, got, loc, _ = device_chain
    poses = got[3]
    used = np.flatnonzero(poses["status"] == 0)
    assert (loc["status"][used] == 0).all()
    for f in used:
        assert np.abs(loc["T"][f][:3, 3] - poses["T"][f][:3, 3]).max() < 1e-5 * LC.TAG_INNER, f
        assert LC.rot_err(loc["T"][f], poses["T"][f]) < 1e-5, f


@pytest.fixture(scope="module")
def webcam_chain():
    """128 frames of test_gpu_calibrate.py's distorted webcam rendered on the device -> detect + PnP with the lens ->
    asl_obs -> map with the lens modelled (n_dist = 5) and without it (n_dist = 0), one stream, read back at the end"""
    import torch
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n, max_tags, w, h, n_ids = 128, 16, CC.WEBCAM_W, CC.WEBCAM_H, 64
    tags, cams = MC.webcam_cameras(n)
    planes, _ = synth.render_planes(w, h, tags, LC.TAG_OUTER, cams, fov_y_deg=CC.WEBCAM_FOV, dist=CC.WEBCAM_DIST)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    Kw = synth.camera_matrix(w, h, CC.WEBCAM_FOV)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    u8 = dict(dtype=torch.uint8, device=dev)
    d_tex = torch.from_numpy(tex).to(dev)
    d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
    frames = torch.empty((n, h, w, 3), **u8)
    d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), **u8)
    out = {}
    bufs = {nd: (torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), **u8), torch.empty((n, CAM_POSE_DTYPE.itemsize), **u8),
                 torch.empty((_lib.MAP_RESULT_DTYPE.itemsize,), **u8)) for nd in (0, 5)}
    torch.cuda.synchronize(dev)
    det.render_frames_device(frames.data_ptr(), n, w, h, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2], tex.shape[1],
                             0.5 * LC.TAG_OUTER, K=Kw, dist=CC.WEBCAM_DIST, stream=st)
    det.submit_device(frames.data_ptr(), n, 3, w, h, stream=st, K=Kw, dist=CC.WEBCAM_DIST, tag_size=LC.TAG_INNER)
    det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=st)
    for nd, (dm, dp, dr) in bufs.items():
        det.build_map_device(d_obs.data_ptr(), n, max_tags, n_ids, Kw, CC.WEBCAM_DIST if nd else None, LC.TAG_INNER, dm.data_ptr(), 0,
                             dp.data_ptr(), dr.data_ptr(), stream=st)
    stream.synchronize()
    for nd, (dm, dp, dr) in bufs.items():
        out[nd] = (dr.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(()), dm.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(n_ids),
                   None, dp.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n))
    obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, max_tags)
    det.collect()
    yield Kw, obs, out, tags, cams
    det.close()


def test_webcam_chain_matches_the_statement_and_the_lens_model_helps(webcam_chain):
    Kw, obs, out, tags, cams = webcam_chain
    want = MR.map_frames(obs, 64, Kw, CC.WEBCAM_DIST, LC.TAG_INNER, with_std=False)[:4]
    assert_same(out[5], want, 1e-7)
    r5, m5, _, p5 = out[5]
    r0, m0, _, p0 = out[0]
    assert r5["status"] == 0 and r0["status"] == 0 and r5["n_frames_used"] >= 100
    assert r5["rms_px"] < 0.5 * r0["rms_px"], (r5["rms_px"], r0["rms_px"])
    e5 = MC.map_errors(m5, p5, tags, cams, int(r5["world_id"]))
    e0 = MC.map_errors(m0, p0, tags, cams, int(r0["world_id"]))
    assert e5[0] < e0[0] and e5[1] < e0[1], (e5, e0)


def test_tag_detector_build_map_from_host_frames():
    import torch

    import bench
    from aprilslam_amd.tag_detector import TagDetector
    dev = torch.device("cuda:0")
    n = 16
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        frames, _, _ = bench.render_stream_device(det, n, dev)
        host = frames.cpu().numpy()
    finally:
        det.close()
    Kr = synth.camera_matrix(LC.W, LC.H, 45.0)
    td = TagDetector({"camera_matrix": Kr, "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER)
    m = td.build_map(list(host))
    assert m.ok, m
    tags = LC.bench_scene()
    res = m.result
    et, er, ec = MC.map_errors(m.records, m.poses, tags, bench.camera_trajectory(n), m.world_id)
    assert et < 0.05 * LC.TAG_INNER and er < 0.01 and ec < 0.1 * LC.TAG_INNER, (et, er, ec)
    assert len(m.tag_map) == int(res["n_tags"]) and set(m.tag_std) == set(m.tag_map.ids())
    assert (m.frame_status == 0).sum() == int(res["n_frames_used"]) and m.camera_poses.shape == (n, 4, 4)
