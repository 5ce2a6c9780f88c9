"""Rig mounting calibration on the device (asl_calibrate_rig_frames_device / asl_calibrate_rig_batch, k_rigcal.inc) against
the NumPy statement (tests/rig_calib_ref.py), against the truth of the motivating case, and end to end on rendered frames.

Bars: the integer fields identical; E and the used frames' T 1e-9 relative on the exact-corner cases and 1e-7 on noisy
corners (the two bars of test_gpu_calibrate.py); rms 1e-6 relative; covariances per element 600 eps kappa
(solver_checks.assert_cov_close), kappa that of the full normal matrix whose inverse the covariance is a block of, against
the dense inverse at the device's own solution.  `iterations` is not compared: a trial accepted on one side and rejected on
the other at rounding level changes the count and not the answer.  On exact corners the cost at the solution is rounding
(rms 2e-5 px), so its estimate of sigma is too: those cases give sigma_px; one_tag estimates it."""
import numpy as np
import pytest

import localize_cases as LC
import rig_calib_cases as CC
import rig_calib_ref as CR
import rig_cases as RC
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap
from aprilslam_amd.rig import Rig, RigCalibrationResult, RigCamera
from solver_checks import assert_cov_close, dev_bytes, rel

pytestmark = pytest.mark.gpu

SIGMA = 0.5
OUT_DTYPES = (_lib.RIG_CAMERA_DTYPE, _lib.RIG_CALIB_RESULT_DTYPE, _lib.POSE_COV_DTYPE, CAM_POSE_DTYPE)


def case_sigma(name):
    return 0.0 if name == "one_tag" else SIGMA


def compare_with_statement(name, obs, rec, rig0, ts, sigma, got, tol):
    """the device's (rig_out, result, cov, poses) against the statement of the same input"""
    out, res, cov, poses = got
    det = {}
    w_out, w_res, w_cov, w_poses = CR.calibrate(obs, rec, rig0, ts, sigma_px=sigma, details=det)
    n = len(out)
    for field in ("status", "n_frames_used", "n_corners", "n_solved"):
        assert res[field] == w_res[field], (field, res[field], w_res[field])
    assert list(res["cam_status"]) == list(w_res["cam_status"]) and list(res["cam_frames"]) == list(w_res["cam_frames"])
    assert res["reserved"] == 0
    assert list(poses["status"]) == list(w_poses["status"]) and list(poses["n_tags"]) == list(w_poses["n_tags"])
    assert list(cov["status"]) == list(w_cov["status"]) and list(cov["dof"]) == list(w_cov["dof"])
    worst_E = max(LC.rel_err(out["E"][k], w_out["E"][k]) for k in range(n))
    used = np.flatnonzero(poses["status"] == 0)
    worst_T = max([LC.rel_err(poses["T"][f], w_poses["T"][f]) for f in used], default=0.0)
    print(name, "status %d, %d frames, %d corners, trials %d (statement %d), E %.2e, T %.2e, rms %.3g -> %.3g px (%.2e, %.2e), sigma %.4g"
          % (res["status"], res["n_frames_used"], res["n_corners"], res["iterations"], w_res["iterations"], worst_E, worst_T, res["rms_init_px"],
             res["rms_px"], rel(res["rms_init_px"], w_res["rms_init_px"]), abs(res["rms_px"] - w_res["rms_px"]) / max(w_res["rms_px"], 1e-300),
             res["sigma_px"]))
    assert worst_E <= tol and worst_T <= tol
    for field in ("rms_px", "rms_init_px", "sigma_px"):
        assert abs(res[field] - w_res[field]) <= 1e-6 * abs(w_res[field]), (field, res[field], w_res[field])
    for f in used:  # a frame's own rms at the float32 floor of exact corners (2e-5 px) is rounding: held from 1e-3 px up
        assert abs(poses["rms_px"][f] - w_poses["rms_px"][f]) <= 1e-6 * max(w_poses["rms_px"][f], 1e-3), f
    assert out["K"].tobytes() == rig0["K"].tobytes() and out["dist"].tobytes() == rig0["dist"].tobytes()
    assert out["n_dist"].tobytes() == rig0["n_dist"].tobytes()
    # cameras that are not solved: E byte for byte, no covariance
    for k in range(n):
        if res["status"] != 0 or res["cam_status"][k] != 0:
            assert out["E"][k].tobytes() == rig0["E"][k].tobytes(), k
            assert cov["status"][k] == 1 and cov["dof"][k] == 0 and not cov["cov"][k].any(), k
        assert cov["sigma_px"][k] == res["sigma_px"], k
    # covariances: the dense inverse of the full normal matrix at the device's own solution
    if res["status"] == 0:
        ref, H = CR.full_normal_cov(obs, rec, out, ts, res, poses, sigma)
        assert sorted(ref) == [k for k in range(n) if cov["status"][k] == 0]
        for k, C in ref.items():
            assert_cov_close(cov["cov"][k], C, H, (name, k))
    return det


@pytest.mark.parametrize("name", CC.NAMES)
def test_kernel_matches_the_statement(gpu_detector, name):
    c = CC.case(name)
    obs, rec, rig0, ts, sigma = c["obs"], c["rec"], c["rig0"].as_records(), c["tag_size"], case_sigma(name)
    got = gpu_detector.calibrate_rig(obs, rec, rig0, ts, sigma_px=sigma)
    compare_with_statement(name, obs, rec, rig0, ts, sigma, got, 1e-9 if c["exact"] or name in ("island", "nothing") else 1e-7)
    out, res, cov, poses = got
    # the frames outside the joint solve: the seed's own record (the device's), status 5 where it was 0
    seed = gpu_detector.localize_rig(obs, rec, rig0, ts)
    outside = np.flatnonzero(poses["status"] != 0)
    for f in outside:
        want = seed[f].copy()
        assert poses["status"][f] == (5 if want["status"] == 0 else want["status"]), f
        want["status"] = poses["status"][f]
        assert poses[f].tobytes() == want.tobytes(), f
    for f in np.flatnonzero(poses["status"] == 0):
        assert poses["seed_slot"][f] == seed["seed_slot"][f] and poses["rms_seed_px"][f] == seed["rms_seed_px"][f] and poses["n_rejected"][f] == 0
    expected_outside = {"dropout": [2, 3], "nothing": list(range(obs.shape[1]))}.get(name, [])
    assert list(outside) == expected_outside
    if name == "island":
        assert list(res["cam_status"][:3]) == [1, 0, 2] and list(cov["status"]) == [1, 0, 1]
    if name == "nothing":
        assert res["status"] == 1 and out.tobytes() == rig0.tobytes()
    if name == "ring8":
        assert res["n_solved"] == 7 and obs.shape[0] * obs.shape[2] == 256


def test_one_small_tag_per_camera_against_the_truth(gpu_detector):
    """Rig.calibrate_mountings on the motivating case: within the truth bound the CPU test fixed for the statement"""
    c = CC.case("one_tag")
    r = c["rig0"].calibrate_mountings(gpu_detector, c["obs"], c["rec"], c["tag_size"])
    assert isinstance(r, RigCalibrationResult) and r.ok and len(r.rig) == 2
    T = c["truth"].cameras[1].T_cam_rig
    rot0, tr0 = CR.mounting_error(c["rig0"].cameras[1].T_cam_rig[:3], T)
    rot, tr = CR.mounting_error(r.rig.cameras[1].T_cam_rig[:3], T)
    std = r.mounting_std()
    print("averaged %.2f deg %.2f units; joint %.4f deg %.4f units, std %s" % (rot0, tr0, rot, tr, np.array2string(std[1], precision=4)))
    assert rot0 > 10.0 and rot <= CC.ONE_TAG_ROT_DEG and tr <= CC.ONE_TAG_TRANS
    assert std.shape == (2, 6) and not std[0].any() and (std[1] > 0).all()
    assert np.array_equal(r.rig.cameras[0].T_cam_rig, c["rig0"].cameras[0].T_cam_rig)


def device_call(det, d_obs, shape, d_map, n_ids, d_rig, ts, sigma, d_rig_out=None, stream=0):
    """one asl_calibrate_rig_frames_device call on zeroed outputs -> the four outputs' bytes (d_rig_out None: its own buffer)"""
    import torch
    dev = d_obs.device
    n_cams, n, mt = shape
    bufs = [torch.zeros(k * dt.itemsize, dtype=torch.uint8, device=dev) for k, dt in zip((n_cams, 1, n_cams, n), OUT_DTYPES)]
    ro = bufs[0] if d_rig_out is None else d_rig_out
    det.calibrate_rig_device(d_obs.data_ptr(), n_cams, n, mt, d_map.data_ptr(), n_ids, d_rig.data_ptr(), ts, ro.data_ptr(), bufs[1].data_ptr(),
                             bufs[2].data_ptr(), bufs[3].data_ptr(), sigma_px=sigma, stream=stream)
    torch.cuda.synchronize()
    return [b.cpu().numpy().tobytes() for b in [ro] + bufs[1:]]


def test_repeated_calls_and_in_place(gpu_detector):
    """the device form on the 8-camera case: the bytes of the host form, the same bytes on every call, and with d_rig_out = d_rig"""
    import torch
    dev = torch.device("cuda:0")
    c = CC.case("ring8")
    obs, rec, rig0, ts = c["obs"], c["rec"], c["rig0"].as_records(), c["tag_size"]
    host = [np.ascontiguousarray(x).tobytes() for x in gpu_detector.calibrate_rig(obs, rec, rig0, ts, sigma_px=SIGMA)]
    d_obs, d_map, d_rig = dev_bytes(obs, dev), dev_bytes(rec, dev), dev_bytes(rig0, dev)
    first = device_call(gpu_detector, d_obs, obs.shape, d_map, len(rec), d_rig, ts, SIGMA)
    assert first == host
    for _ in range(2):
        assert device_call(gpu_detector, d_obs, obs.shape, d_map, len(rec), d_rig, ts, SIGMA) == first
    assert d_rig.cpu().numpy().tobytes() == rig0.tobytes()
    in_place = device_call(gpu_detector, d_obs, obs.shape, d_map, len(rec), d_rig, ts, SIGMA, d_rig_out=d_rig)
    assert in_place == first


# ---- end to end on the device

E2E_FRAMES, E2E_MAX_TAGS = 32, 32
K = synth.camera_matrix(LC.W, LC.H, 45.0)


# The rendered chain's check against the renderer's mounting.  Both estimates rest on the same detector corners, so each is
# off the truth by about the first-order uncertainty of such an estimate: the refined one cannot be asked to be nearer in a
# single draw, but it must not be further than the averaged one by more than that uncertainty explains.  Allowance: 2
# (the usual two sigma, fixed before the first device run of this check) times the std of the error's norm that the solve
# reports for itself, sqrt(trace) of the rotation and of the translation block of camera 1's covariance.
MOUNTING_SIGMAS = 2.0


def test_device_chain_from_rendered_frames():
    """The recipe of test_gpu_rig.rig_block at 32 frames: two streams rendered on the device, detected and packed into one
    block, each camera localised alone (one read-back, for Rig.from_camera_poses on the host), then the averaged mountings
    go back to the device and asl_calibrate_rig_frames_device refines them on the same stream (one read-back of the results).
    Against the statement at 1e-7 (detector corners), and against the renderer's mounting E1: the refined mounting's
    rotation error (angle of E E1^-1) and translation error (|te - te1|) are each no larger than the averaged mounting's
    plus MOUNTING_SIGMAS reported std of that error (see there); all figures are printed."""
    import torch

    import bench
    dev = torch.device("cuda:0")
    n, mt = E2E_FRAMES, E2E_MAX_TAGS
    tags = LC.bench_scene()
    rec = TagMap.from_scene(tags).as_records()
    E1 = RC.mounting(8.0, (6.0, 0.5, 0.0), 1.0)
    cams0 = bench.camera_trajectory(n)
    truth = [LC.world_from_camera(p, r) for p, r in cams0]
    cams = [cams0, [RC.synth_camera(T @ np.linalg.inv(E1)) for T in truth]]
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    d_tex = torch.from_numpy(tex).to(dev)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_obs = torch.empty((2, n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map = dev_bytes(rec, dev)
    d_single = torch.empty((2, n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    dets, keep = [], []
    try:
        for c in range(2):
            det = _lib.Detector("tagStandard41h12", id_limit=0)
            dets.append(det)
            planes, _ = synth.render_planes(LC.W, LC.H, tags, LC.TAG_OUTER, cams[c])
            d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
            frames = torch.empty((n, LC.H, LC.W, 3), dtype=torch.uint8, device=dev)
            keep += [d_planes, frames]
            det.render_frames_device(frames.data_ptr(), n, LC.W, LC.H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2],
                                     tex.shape[1], 0.5 * LC.TAG_OUTER, stream=st)
            det.submit_device(frames.data_ptr(), n, 3, LC.W, LC.H, stream=st, K=K, dist=np.zeros(4), tag_size=LC.TAG_INNER)
            det.pack_observations_device(d_obs[c].data_ptr(), mt, stream=st)
        det = dets[0]
        for c in range(2):
            det.localize_device(d_obs[c].data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_single[c].data_ptr(), K, None, LC.TAG_INNER, stream=st)
        stream.synchronize()
        single = d_single.cpu().numpy().view(CAM_POSE_DTYPE).reshape(2, n)
        rig0 = Rig.from_camera_poses([(K, None), (K, None)], [single[0], single[1]])
        rig0_rec = rig0.as_records()
        d_rig = dev_bytes(rig0_rec, dev)
        outs = [torch.zeros(k * dt.itemsize, dtype=torch.uint8, device=dev) for k, dt in zip((2, 1, 2, n), OUT_DTYPES)]
        det.calibrate_rig_device(d_obs.data_ptr(), 2, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), LC.TAG_INNER, outs[0].data_ptr(),
                                 outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), stream=st)
        stream.synchronize()
        got = [o.cpu().numpy().view(dt) for o, dt in zip(outs, OUT_DTYPES)]
        got[1] = got[1].reshape(())
        obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(2, n, mt)
        for d in dets:
            d.collect()
    finally:
        for d in dets:
            d.close()
    out, res, cov, poses = got
    assert res["status"] == 0 and res["n_frames_used"] == n and (poses["status"] == 0).all() and res["n_corners"] >= 4 * 20 * n
    compare_with_statement("rendered", obs, rec, rig0_rec, LC.TAG_INNER, 0.0, got, 1e-7)
    avg = CR.mounting_error(rig0_rec["E"][1], E1)
    ref = CR.mounting_error(out["E"][1], E1)
    C = cov["cov"][1]
    std_rot, std_tr = float(np.degrees(np.sqrt(np.trace(C[:3, :3])))), float(np.sqrt(np.trace(C[3:, 3:])))
    print("camera 1's mounting against the renderer's: averaged %.5f deg %.5f units; refined %.5f deg %.5f units; reported std of the error "
          "%.5f deg %.5f units (sigma %.4f px, dof %d)" % (avg + ref + (std_rot, std_tr, res["sigma_px"], cov["dof"][1])))
    assert cov["status"][1] == 0 and std_rot > 0 and std_tr > 0
    assert ref[0] <= avg[0] + MOUNTING_SIGMAS * std_rot, (ref[0], avg[0], std_rot)
    assert ref[1] <= avg[1] + MOUNTING_SIGMAS * std_tr, (ref[1], avg[1], std_tr)


# ---- the ABI

def test_errors_are_loud_and_write_nothing(gpu_detector):
    import torch
    dev = torch.device("cuda:0")
    L = _lib.load()
    c = CC.case("pair")
    obs, rec, rig = np.ascontiguousarray(c["obs"]), c["rec"], c["rig0"].as_records()
    n_cams, n, mt = obs.shape
    d_obs, d_map, d_rig = dev_bytes(obs, dev), dev_bytes(rec, dev), dev_bytes(rig, dev)
    skew = rig["E"][1].copy()
    skew[0, 0] += 1e-4

    def bad_table(field, value, cam=1):
        r = rig.copy()
        r[field][cam] = value
        return r

    tables = [bad_table("n_dist", 3), bad_table("K", np.full((3, 3), np.nan)), bad_table("E", np.full((3, 4), np.inf), 0), bad_table("E", skew)]
    bad = [dict(obs=None), dict(map=None), dict(rig=None), dict(rig_out=None), dict(result=None), dict(cov=None), dict(poses=None),
           dict(n_cams=1), dict(n_cams=9), dict(n_cams=0), dict(max_tags=0), dict(max_tags=257), dict(n_cams=8, max_tags=33), dict(n_frames=0),
           dict(n_frames=-1), dict(n_ids=0), dict(tag_size=0.0), dict(tag_size=-1.0), dict(tag_size=float("nan")), dict(tag_size=float("inf")),
           dict(max_iters=0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf"))]
    sizes = (n_cams, 1, n_cams, n)
    keep = []
    for device in (True, False):
        if device:
            outs = [torch.full((k * dt.itemsize,), 0x55, dtype=torch.uint8, device=dev) for k, dt in zip(sizes, OUT_DTYPES)]
            ptrs = [o.data_ptr() for o in outs]
            base = dict(obs=d_obs.data_ptr(), map=d_map.data_ptr(), rig=d_rig.data_ptr())
        else:
            outs = [np.full(k * dt.itemsize, 0x55, dtype=np.uint8) for k, dt in zip(sizes, OUT_DTYPES)]
            ptrs = [o.ctypes.data for o in outs]
            base = dict(obs=obs.ctypes.data, map=rec.ctypes.data, rig=rig.ctypes.data)
        base.update(n_cams=n_cams, n_frames=n, max_tags=mt, n_ids=len(rec), tag_size=c["tag_size"], max_iters=30, sigma=0.5, rig_out=ptrs[0],
                    result=ptrs[1], cov=ptrs[2], poses=ptrs[3])
        variants = [dict(base, **b) for b in bad]
        for t in tables:
            tab = dev_bytes(t, dev) if device else np.ascontiguousarray(t)
            keep.append(tab)
            variants.append(dict(base, rig=tab.data_ptr() if device else tab.ctypes.data))
        for a in variants:
            args = (gpu_detector._h, a["obs"], a["n_cams"], a["n_frames"], a["max_tags"], a["map"], a["n_ids"], a["rig"], a["tag_size"], a["max_iters"],
                    a["sigma"], a["rig_out"], a["result"], a["cov"], a["poses"])
            rc = L.asl_calibrate_rig_frames_device(*args, None) if device else L.asl_calibrate_rig_batch(*args)
            assert rc == -1, (device, {k: v for k, v in a.items() if base.get(k) != v})
            assert len(L.asl_last_error()) > 0
        if device:
            torch.cuda.synchronize()
            assert all(bool((o == 0x55).all()) for o in outs)
        else:
            assert all((o == 0x55).all() for o in outs)
    assert L.asl_calibrate_rig_batch(None, obs.ctypes.data, n_cams, n, mt, rec.ctypes.data, len(rec), rig.ctypes.data, c["tag_size"], 30, 0.0,
                                     ptrs[0], ptrs[1], ptrs[2], ptrs[3]) == -1
    # the Python surface raises, with the library's message
    with pytest.raises(_lib.AslError, match="n_cams"):
        gpu_detector.calibrate_rig(obs[:1], rec, rig[:1], c["tag_size"])
    with pytest.raises(_lib.AslError, match="max_iters"):
        gpu_detector.calibrate_rig(obs, rec, rig, c["tag_size"], max_iters=0)
    with pytest.raises(_lib.AslError, match="sigma_px"):
        gpu_detector.calibrate_rig(obs, rec, rig, c["tag_size"], sigma_px=-1.0)
    with pytest.raises(_lib.AslError, match="tag_size"):
        gpu_detector.calibrate_rig(obs, rec, rig, 0.0)
    with pytest.raises(_lib.AslError, match="rotation"):
        gpu_detector.calibrate_rig(obs, rec, tables[3], c["tag_size"])
    with pytest.raises(_lib.AslError, match="max_tags"):
        gpu_detector.calibrate_rig_device(d_obs.data_ptr(), n_cams, n, 0, d_map.data_ptr(), len(rec), d_rig.data_ptr(), c["tag_size"], *ptrs)
    with pytest.raises(ValueError):
        gpu_detector.calibrate_rig(obs, rec, rig[:1], c["tag_size"])
    with pytest.raises(ValueError):
        c["rig0"].calibrate_mountings(gpu_detector, obs[:1], rec, c["tag_size"])
    with pytest.raises(ValueError):
        Rig([RigCamera(K)]).calibrate_mountings(gpu_detector, obs[:1], rec, c["tag_size"])
