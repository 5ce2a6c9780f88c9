"""Sequence localisation on the device (asl_smooth_frames_device / asl_smooth_batch, k_smooth.inc) against the NumPy
statement (tests/smooth_ref.py) on the cases and recorded figures of tests/smooth_cases.py."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_ref as SR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in SC.all_cases()}


def device(det, name, seed="given"):
    obs, rec, sd, dist, sig, iters = CASES[name]
    return det.smooth(obs, rec, SC.K, dist, SC.TAG, *sig, max_iters=iters, seed=sd if seed == "given" else None)


def close(a, b, rel):
    return abs(a - b) <= rel * max(1.0, abs(b))


def assert_same(name, got, gres):
    """every field of the device's records against the statement's"""
    want, wres, trace = SC.statement(name)
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d / %d, cost %.12g / %.12g" %
          (name, worst, SC.DEVICE_TOL, gres["iterations"], wres["iterations"], gres["cost"], wres["cost"]))
    for k in ("status", "n_tags", "n_rejected"):
        assert np.array_equal(got[k], want[k]), (name, k)
    for k in ("n_frames_data", "n_filled", "status", "iterations"):
        assert gres[k] == wres[k], (name, k, gres[k], wres[k])
    assert not np.any(gres["reserved"])
    if not np.array_equal(got["seed_slot"], want["seed_slot"]):
        # a different candidate somewhere: only where the two chains cost the same to 1e-9 (the seeds' tie rule)
        posed = trace["posed"]
        choice = np.array([1 if got["seed_slot"][f] != CASES[name][2]["seed_slot"][f] else 0 for f in posed])
        assert all(got["seed_slot"][f] in (CASES[name][2]["seed_slot"][f], CASES[name][2]["seed_slot"][f] + SR.FLIPPED) for f in posed)
        a, b = SR.chain_total(trace["d"], trace["tr"], choice), SR.chain_total(trace["d"], trace["tr"], trace["choice"])
        assert abs(a - b) <= 1e-9 * max(1.0, b), (name, a, b)
    else:
        assert gres["n_flipped"] == wres["n_flipped"]
    assert worst <= SC.DEVICE_TOL, (name, worst)
    for k in ("rms_px", "rms_seed_px"):
        assert all(close(g, w, 1e-6) for g, w in zip(got[k], want[k])), (name, k)
        assert close(gres[k], wres[k], 1e-6), (name, k)
    for k in ("cost", "cost_seed"):
        assert abs(gres[k] - wres[k]) <= 1e-6 * max(1.0, abs(wres[k])), (name, k, gres[k], wres[k])


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_device_matches_the_statement(gpu_detector, shape):
    name = "shape%d_%d_%d" % shape
    assert_same(name, *device(gpu_detector, name))


def scene(det, name, same_trials):
    """a converged scene on the device: statuses and flip marks as the statement's, and the solve stopped by itself.
    same_trials: also the number of trials and T within DEVICE_TOL -- for the scenes whose trial count the statement keeps
    under the rounding perturbation of test_smooth_ref.test_device_tolerance_and_chain_margins (holes, noise).  The one-tag
    scenes have no slot order to perturb, so the statement cannot show that for them; their tail of trials at the converged
    pose is decided by rounding (smooth_cases.COMPARE_ITERS), and their poses are held to the truth by the recorded figures."""
    got, res = device(det, name)
    want, wres, _ = SC.statement(name)
    assert 1 <= res["iterations"] < SC.MAX_ITERS and 1 <= wres["iterations"] < SC.MAX_ITERS    # stopped, not run out
    if same_trials:
        assert res["iterations"] == wres["iterations"], (name, res["iterations"], wres["iterations"])
        assert max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"])) <= SC.DEVICE_TOL
        assert all(close(g, w, 1e-6) for g, w in zip(got["rms_px"], want["rms_px"]))
    print("%s: T rel_err %.3g, trials %d / %d, cost %.12g / %.12g" % (name, max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"])),
                                                                   res["iterations"], wres["iterations"], res["cost"], wres["cost"]))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), (name, k)
    for k in ("n_frames_data", "n_filled", "n_flipped", "status"):
        assert res[k] == wres[k], (name, k)
    assert close(res["cost_seed"], wres["cost_seed"], 1e-6) and close(res["cost"], wres["cost"], 1e-6)
    return got, res


def test_holes_on_the_device(gpu_detector):
    got, res = scene(gpu_detector, "holes", True)
    truth = SC.holes()[3]
    assert got["status"].tolist() == [6, 0, 0, 6, 0, 0, 6]
    err = SC.pos_err(got["T"], truth)
    assert max(err[0], err[6]) <= 2 * SC.recorded()["holes_end_err"] and err[3] <= 2 * SC.recorded()["holes_mid_err"], err


@pytest.mark.parametrize("first", [False, True])
def test_flips_on_the_device(gpu_detector, first):
    name = "flips_first" if first else "flips"
    got, res = scene(gpu_detector, name, False)
    seed, frames = SC.flips(first)[2], SC.flips(first)[4]
    assert np.flatnonzero(got["seed_slot"] == seed["seed_slot"] + SR.FLIPPED).tolist() == list(frames) and res["n_flipped"] == len(frames)
    final, seeds = SC.flip_errors(got["T"], first)
    assert final <= 2 * SC.recorded()["flips_first_margin" if first else "flips_margin"] * seeds, (final, seeds)


def test_noise_on_the_device(gpu_detector):
    got, res = scene(gpu_detector, "noise", True)
    truth = SC.noise()[3]
    smooth = float(np.sqrt(np.mean(SC.pos_err(got["T"], truth) ** 2)))
    assert smooth <= 2 * SC.recorded()["noise_rmse_smooth"] and smooth < SC.recorded()["noise_rmse_frame"], smooth


@pytest.mark.parametrize("name", ["all_empty", "first_only", "last_only", "hole70", "one_id"])
def test_edge_sequences(gpu_detector, name):
    got, res = device(gpu_detector, name)
    assert_same(name, got, res)
    if name == "all_empty":
        assert res["status"] == 1 and (got["status"] == 1).all() and all(np.array_equal(T, np.eye(4)) for T in got["T"])
        assert (got["seed_slot"] == -1).all() and res["iterations"] == 0
    if name == "hole70":
        assert (got["status"][2:72] == 6).all() and res["n_filled"] == 70


@pytest.mark.parametrize("name", ["behind", "nonfinite"])
def test_solves_that_fail(gpu_detector, name):
    """no positive pivot in any trial (result status 2) and a non-finite cost after the chain (status 3): frames status 4"""
    obs, rec, seed, sig, iters, status, trials = SC.failure_cases()[name]
    got, res = gpu_detector.smooth(obs, rec, SC.K, None, SC.TAG, *sig, max_iters=iters, seed=seed)
    want, wres, _ = SC.run(obs, rec, seed, None, sig, max_iters=iters)
    assert res["status"] == status == wres["status"] and res["iterations"] == trials == wres["iterations"]
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["status"] == 4).all()
    for k in ("n_frames_data", "n_filled", "n_flipped"):
        assert res[k] == wres[k], k
    if name == "behind":
        assert LC.rel_err(got["T"][0], want["T"][0]) <= SC.DEVICE_TOL and close(res["cost"], wres["cost"], 1e-6) and res["cost"] == res["cost_seed"]
    else:
        assert not np.isfinite(res["cost_seed"]) and LC.rel_err(got["T"][0], want["T"][0]) <= SC.DEVICE_TOL


@pytest.fixture(scope="module")
def on_device(gpu_detector):
    """the 65-frame case on device buffers: localisation and smoothing enqueued on one stream, no host wait between them"""
    import torch
    dev = torch.device("cuda:0")
    obs, rec, _, dist, sig, iters = CASES["shape65_4_5"]
    n, mt = obs.shape
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(-1)).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_seed = torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(_lib.SMOOTH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)

    def run():
        d_out.zero_()
        d_res.zero_()
        torch.cuda.synchronize()
        gpu_detector.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), SC.K, dist, SC.TAG,
                                     stream=stream.cuda_stream)
        gpu_detector.smooth_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                   SC.K, dist, SC.TAG, *sig, max_iters=iters, stream=stream.cuda_stream)
        stream.synchronize()
        return d_out.cpu().numpy().tobytes(), d_res.cpu().numpy().tobytes()
    return run, (d_obs, d_map, d_seed, d_out, d_res, n, mt, len(rec), dist, sig)


def test_both_entry_points_agree_byte_for_byte(gpu_detector, on_device):
    run, _ = on_device
    out_b, res_b = run()
    got, res = device(gpu_detector, "shape65_4_5", seed=None)     # asl_smooth_batch with seed == NULL
    assert got.tobytes() == out_b and res.tobytes() == res_b
    assert res["status"] == 0 and (np.isin(got["status"], (0, 6))).all()


def test_the_same_input_gives_the_same_bytes(on_device):
    run, _ = on_device
    assert run() == run()


def test_refused_arguments_write_nothing(gpu_detector, on_device):
    import torch
    _, (d_obs, d_map, d_seed, d_out, d_res, n, mt, n_ids, dist, sig) = on_device
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    Kc, dc = np.ascontiguousarray(SC.K), np.ascontiguousarray(dist)
    ok = [gpu_detector._h, d_obs.data_ptr(), n, mt, d_map.data_ptr(), n_ids, Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, SC.TAG,
          d_seed.data_ptr(), sig[0], sig[1], sig[2], 5, d_out.data_ptr(), d_res.data_ptr(), None]
    Knan = Kc.copy()
    Knan[0, 0] = np.nan
    nan, inf = float("nan"), float("inf")
    bad = [(1, None), (4, None), (6, None), (10, None), (15, None), (16, None), (2, 0), (2, 65536), (3, 0), (3, 257), (8, 3), (7, None),
           (6, Knan.ctypes.data_as(dp)), (9, nan), (9, inf), (11, 0.0), (11, nan), (12, -1.0), (12, inf), (13, 0.0), (13, nan), (14, 0), (14, 101),
           (15, d_seed.data_ptr()), (15, d_seed.data_ptr() + 160 * (n - 1))]
    d_out.fill_(0xAB)
    d_res.fill_(0xAB)
    seed_before = d_seed.cpu().numpy().tobytes()
    torch.cuda.synchronize()
    for k, v in bad:
        a = list(ok)
        a[k] = v
        assert L.asl_smooth_frames_device(*a) == -1, (k, v)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xAB).all() and (d_res.cpu().numpy() == 0xAB).all() and d_seed.cpu().numpy().tobytes() == seed_before
    assert L.asl_smooth_frames_device(*ok) == 0
    torch.cuda.synchronize()
    assert not (d_res.cpu().numpy() == 0xAB).all()
    # the host form refuses the same way
    obs, rec = CASES["shape65_4_5"][:2]
    out = np.full(n, 0xAB, dtype=np.uint8).repeat(CAM_POSE_DTYPE.itemsize)
    res = np.full(64, 0xAB, dtype=np.uint8)
    hk = [gpu_detector._h, obs.ctypes.data, n, mt, rec.ctypes.data, n_ids, Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, SC.TAG, None,
          sig[0], sig[1], sig[2], 5, out.ctypes.data, res.ctypes.data]
    for k, v in ((1, None), (4, None), (6, None), (15, None), (16, None), (2, 0), (3, 257), (8, 2), (11, -1.0), (13, nan), (14, 0)):
        a = list(hk)
        a[k] = v
        assert L.asl_smooth_batch(*a) == -1, (k, v)
    assert (out == 0xAB).all() and (res == 0xAB).all()


def test_tag_detector_and_slam_surface():
    """TagDetector.localize_sequence on what detect_host returns: three rendered frames around a blank one"""
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.smooth import SmoothResult
    from aprilslam_amd.tag_detector import TagDetector
    from aprilslam_amd.localize import TagMap
    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, id_limit=0)
    cams = LC.trajectory(520)[:3]
    frames = [synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r)[0] for p, r in cams]
    frames.insert(2, np.zeros_like(frames[0]))
    d, p, npf = td.detector._det.detect_host(np.stack(frames), K=SC.K, dist=np.zeros(4), tag_size=SC.TAG)
    r = td.localize_sequence(d, p, npf, tm, sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2)
    assert isinstance(r, SmoothResult) and r.ok and r.trajectory().shape == (4, 4, 4)
    assert r.poses["status"].tolist() == [0, 0, 6, 0] and r.filled.tolist() == [False, False, True, False] and not r.flipped.any()
    assert r.prior_only.tolist() == [False, False, True, False]
    truth = [LC.world_from_camera(*c) for c in cams]
    for T, t in zip(r.trajectory()[[0, 1, 3]], truth):
        assert LC.rot_err(T, t) <= 2e-3 and np.linalg.norm(T[:3, 3] - t[:3, 3]) <= 0.25
    assert np.linalg.norm(r.trajectory()[2][:3, 3] - truth[1][:3, 3]) <= 0.25     # the blank frame sits with its neighbours

    class _Log:
        def info(self, m):
            pass
    slam = SLAM(_Log(), {"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, detector=td)
    for det in slam.detect(frames[0]):
        slam.get_pose(det)
    before = slam.graph.estimated_pose.copy()
    rs = slam.localize_sequence(d, p, npf, sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2)
    assert rs.ok and rs.trajectory().shape == (4, 4, 4) and np.array_equal(slam.graph.estimated_pose, before)
