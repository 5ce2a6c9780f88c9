"""Per-tag sizes in the tag map on the device: every solver that takes a map (localisation of one camera and of a rig, their
covariances, calibration, the sequence solves) against its NumPy statement (the size rule: tests/localize_ref.py) on the
cases of tests/sized_cases.py, against the truth, and end to end on rendered frames.

Bars, taken from the tests of the same comparison over equal-size maps: pose 1e-9 relative, rms 1e-6, counts, statuses and
seeds identical or of equal score (test_gpu_localize.assert_same, test_gpu_rig); covariance per element 600 eps kappa
(solver_checks.assert_cov_close); calibration 1e-9 (test_gpu_calibrate.assert_same); the sequence solves 1e-9 after
smooth_cases.COMPARE_ITERS trials (test_gpu_smooth_rig.assert_same); detector corners 1e-7 (test_gpu_localize's device block)."""
import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import rig_ref as RR
import sized_cases as ZC
import smooth_cov_ref as SV
import smooth_ref as SR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap
from solver_checks import assert_cov_close, dev_bytes, rel

pytestmark = pytest.mark.gpu

K, TAG, SIGMA = ZC.K, ZC.TAG, ZC.SIGMA


def localize_device(det, obs, rec, dist, tag_size, gate=0.0, sigma_px=None):
    """asl_localize[_cov]_frames_device on host arrays -> poses[, covariances]"""
    import torch
    dev = torch.device("cuda:0")
    n, mt = obs.shape
    d_obs, d_map = dev_bytes(obs, dev), dev_bytes(rec, dev)
    d_out = torch.full((n * CAM_POSE_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
    d_cov = None if sigma_px is None else torch.full((n * POSE_COV_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
    det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, dist, tag_size, max_tag_rms_px=gate,
                        stream=torch.cuda.current_stream().cuda_stream, cov_ptr=None if d_cov is None else d_cov.data_ptr(),
                        sigma_px=0.0 if sigma_px is None else sigma_px)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    return out if d_cov is None else (out, d_cov.cpu().numpy().view(POSE_COV_DTYPE).reshape(n))


def assert_loc_same(got, want, obs, rec, dist, tag_size=TAG, tol=1e-9, Kc=K):
    """test_gpu_localize.assert_same over a sized map"""
    for f, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"] and g["n_tags"] == w["n_tags"] and g["n_rejected"] == w["n_rejected"], f
        assert LC.rel_err(g["T"], w["T"]) <= tol, (f, LC.rel_err(g["T"], w["T"]))
        assert abs(g["rms_px"] - w["rms_px"]) <= 1e-6 * max(1.0, w["rms_px"])
        assert abs(g["rms_seed_px"] - w["rms_seed_px"]) <= 1e-6 * max(1.0, w["rms_seed_px"])
        if g["seed_slot"] != w["seed_slot"]:
            sc = LR.candidate_scores(LR.OneCamera(LR.camera(Kc, dist)), obs[f], rec, tag_size)
            assert g["seed_slot"] in sc and abs(sc[g["seed_slot"]] - sc[w["seed_slot"]]) <= 1e-9 * max(1.0, sc[w["seed_slot"]]), (f, g["seed_slot"], w["seed_slot"])


def assert_loc_cov(model, frames, rec, out, cov, traces, sigma_px):
    """test_gpu_pose_cov.check_localize_cov: the statement at the device's own pose on the statement's active set"""
    for f, (g, c) in enumerate(zip(out, cov)):
        if g["status"] != 0:
            assert c["status"] == 1 and c["dof"] == 0 and c["sigma_px"] == sigma_px and not c["cov"].any(), f
            continue
        Xw, uv, ci = LR.frame_points(model, frames[f], rec, TAG, traces[f]["active"])
        R = g["T"][:3, :3].T
        t = -(R @ g["T"][:3, 3])
        ref, sig, dof, status = LR.pose_cov(model, R, t, Xw, uv, ci, sigma_px)
        assert status == 0 and c["status"] == 0 and c["dof"] == dof == 8 * g["n_tags"] - 6 and c["sigma_px"] == sig, f
        assert_cov_close(c["cov"], ref, model.linearise(R, t, Xw, uv, ci)[1], f)


# ---- 1: fails without the feature

def test_mixed_size_scene_is_solved_to_the_truth(gpu_detector):
    """test_sized_ref's truth case through asl_localize_batch and asl_localize_frames_device, to the bar measured there with
    the statement (6.46e-05 here); a library that ignores the size misses it by five orders of magnitude"""
    base, bar = ZC.truth_bar()
    obs, rec, truths = ZC.truth_case()
    host = gpu_detector.localize(obs, rec, K, None, TAG)
    devf = localize_device(gpu_detector, obs, rec, None, TAG)
    for name, got in (("host", host), ("device", devf)):
        err = ZC.truth_err(got, truths)
        print("%s form: error against the truth %.3g, bar %.3g" % (name, err, bar))
        assert (got["status"] == 0).all() and (got["n_tags"] == 4).all() and (got["n_rejected"] == 0).all()
        assert err <= bar, (name, err, bar)
    assert host.tobytes() == devf.tobytes()


# ---- 2: kernel against statement

@pytest.mark.parametrize("max_tags", ZC.LOC_MAX_TAGS)
def test_localize_matches_the_statement(gpu_detector, max_tags):
    """plain and with covariance on sized_cases.loc_case: a sized winner, its mirrored candidate, the gate's drop of a sized
    slot, a sized tag alone, slot 64 sized at max_tags 65 (what each frame is for is asserted of the statement on the CPU)"""
    obs, rec, dist, notes = ZC.loc_case(max_tags)
    plain = gpu_detector.localize(obs, rec, K, dist, TAG, max_tag_rms_px=ZC.GATE)
    out, cov = gpu_detector.localize(obs, rec, K, dist, TAG, max_tag_rms_px=ZC.GATE, sigma_px=SIGMA)
    assert out.tobytes() == plain.tobytes()
    traces = []
    want = LR.localize(obs, rec, K, dist, TAG, ZC.GATE, traces=traces)
    print("max_tags %d: T rel_err per frame %s, seeds %s" % (max_tags, ["%.2g" % LC.rel_err(g["T"], w["T"]) for g, w in zip(out, want)],
                                                             out["seed_slot"].tolist()))
    assert_loc_same(out, want, obs, rec, dist)
    assert out["seed_slot"][1] in notes[1] and out["seed_slot"][2] - LR.MIRRORED in notes[2]
    assert out["n_rejected"].tolist() == want["n_rejected"].tolist() and out["n_rejected"][3] == (1 if max_tags >= 2 else 0)
    assert_loc_cov(LR.OneCamera(LR.camera(K, dist)), obs, rec, out, cov, traces, SIGMA)


def test_rig_matches_the_statement(gpu_detector):
    """2 cameras, max_tags 3, 6 frames, the sized tag only in camera 1 in frames 2 to 4; test_gpu_rig's comparison"""
    obs, rec, rig = ZC.rig_case()
    plain = rig.localize(gpu_detector, obs, rec, TAG, 0.0)
    out, cov = rig.localize(gpu_detector, obs, rec, TAG, 0.0, with_cov=True, sigma_px=SIGMA)
    assert out.tobytes() == plain.tobytes()
    traces = []
    want = RR.localize(obs, rec, rig, TAG, 0.0, traces=traces)
    for f, (g, w) in enumerate(zip(out, want)):
        print("rig", f, "pose %.2e rms %.2e seed rms %.2e" % (LC.rel_err(g["T"], w["T"]), rel(g["rms_px"], w["rms_px"]), rel(g["rms_seed_px"], w["rms_seed_px"])))
        for field in ("status", "n_tags", "n_rejected", "seed_slot"):
            assert g[field] == w[field], (f, field, g[field], w[field])
        assert LC.rel_err(g["T"], w["T"]) <= 1e-9, (f, LC.rel_err(g["T"], w["T"]))
        assert rel(g["rms_px"], w["rms_px"]) <= 1e-9 and rel(g["rms_seed_px"], w["rms_seed_px"]) <= 1e-9, f
        assert g["status"] == 0
    assert_loc_cov(RR.RigModel(rig), [obs[:, f] for f in range(obs.shape[1])], rec, out, cov, traces, SIGMA)


def close(a, b, r=1e-6):
    return abs(a - b) <= r * max(1.0, abs(b))


def assert_smooth_same(name, got, gres, want, wres, tol=1e-9):
    """test_gpu_smooth_rig.assert_same"""
    worst = max(LC.rel_err(g, w) for g, w in zip(got["T"], want["T"]))
    print("%s: T rel_err %.3g (bound %.3g), trials %d / %d, cost %.12g / %.12g" % (name, worst, tol, gres["iterations"], wres["iterations"],
                                                                                 gres["cost"], wres["cost"]))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    for k in ("n_frames_data", "n_filled", "n_flipped", "status", "iterations", "n_soft"):
        assert gres[k] == wres[k], (name, k, gres[k], wres[k])
    assert worst <= tol, (name, worst)
    for k in ("rms_px", "rms_seed_px"):
        assert all(close(g, w) for g, w in zip(got[k], want[k])), (name, k)
        assert close(gres[k], wres[k]), (name, k)
    for k in ("cost", "cost_seed"):
        assert close(gres[k], wres[k]), (name, k, gres[k], wres[k])


HUBER_PX = 0.3     # corners with 0.2 px noise: some residuals are over it


@pytest.mark.parametrize("huber", [0.0, HUBER_PX])
def test_sequence_solve_matches_the_statement(gpu_detector, huber):
    """12 frames, max_tags 3: frames without a tag, frames of one sized tag alone (candidate B), one seed mirrored"""
    obs, rec, seed = ZC.smooth_case()
    got, gres = gpu_detector.smooth(obs, rec, K, None, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed, huber_px=huber)
    want, wres, _ = SR.smooth(obs, rec, K, None, TAG, seed, *ZC.SMOOTH_SIGMAS, ZC.SMOOTH_ITERS, huber_px=huber)
    assert want["status"].tolist() == [0, 0, 6, 0, 0, 0, 6, 0, 0, 0, 0, 0] and wres["n_flipped"] >= 1
    assert (wres["n_soft"] > 0) == (huber > 0)
    assert_smooth_same("smooth huber %g" % huber, got, gres, want, wres)


def test_sequence_solve_with_covariance(gpu_detector):
    obs, rec, seed = ZC.smooth_case()
    plain, pres = gpu_detector.smooth(obs, rec, K, None, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed)
    out, res, cov = gpu_detector.smooth(obs, rec, K, None, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed, with_cov=True)
    assert out.tobytes() == plain.tobytes() and res.tobytes() == pres.tobytes()
    want, A = SV.smooth_cov(obs, rec, K, None, TAG, out, res, *ZC.SMOOTH_SIGMAS)
    assert res["status"] == 0 and (want["status"] == 0).all()
    for k in ("status", "dof", "sigma_px"):
        assert np.array_equal(cov[k], want[k]), (k, cov[k], want[k])
    for f in range(len(out)):
        assert_cov_close(cov["cov"][f], want["cov"][f], A, f)


def test_rig_sequence_solve_matches_the_statement(gpu_detector):
    """2 cameras x 8 frames"""
    obs, rec, rig, seed = ZC.smooth_rig_case()
    got, gres = gpu_detector.smooth_rig(obs, rec, rig, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed)
    want, wres, _ = SR.smooth_rig(obs, rec, rig, TAG, seed, *ZC.SMOOTH_SIGMAS, ZC.SMOOTH_ITERS)
    assert want["status"].tolist() == [0, 0, 0, 6, 0, 0, 0, 0]
    assert_smooth_same("smooth rig", got, gres, want, wres)


@pytest.mark.parametrize("n_dist", [0, 5])
def test_calibration_matches_the_statement(gpu_detector, n_dist):
    """a board of two tag sizes, 6 frames; the fields and bars of test_gpu_calibrate.assert_same at its 1e-9"""
    import calib_cases as CC
    import calib_ref as CR
    obs, rec = ZC.calib_case(n_dist)
    got = gpu_detector.calibrate(obs, rec, TAG, CC.W, CC.H, n_dist=n_dist)
    want = CR.calibrate(obs, rec, TAG, CC.W, CC.H, n_dist=n_dist)
    print("calibration n_dist %d: K %s rms %.3g" % (n_dist, got[0]["K"].ravel()[[0, 4, 2, 5]], got[0]["rms_px"]))
    assert want[0]["status"] == 0 and want[0]["rms_px"] < 1e-3        # the two sizes are honoured: exact corners fit
    (gr, gp), (wr, wp), tol = got, want, 1e-9

    def rel_max(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return float(np.abs(x - y).max() / max(1e-300, np.abs(y).max()))
    assert gr["status"] == wr["status"] and gr["n_frames_used"] == wr["n_frames_used"] and gr["n_corners"] == wr["n_corners"]
    assert np.array_equal(gp["status"], wp["status"]) and np.array_equal(gp["n_tags"], wp["n_tags"])
    assert rel_max(gr["K"], wr["K"]) <= tol, (gr["K"], wr["K"])
    assert np.abs(gr["dist"] - wr["dist"]).max() <= tol * max(1.0, np.abs(wr["dist"]).max())
    assert np.array_equal(gr["std"] == 0, wr["std"] == 0)
    assert rel_max(gr["std"], wr["std"]) <= max(tol, 1e-7), (gr["std"], wr["std"])   # a ratio of small sums: a few digits fewer
    for g, w in zip(gp, wp):
        assert LC.rel_err(g["T"], w["T"]) <= tol
    assert abs(gr["rms_px"] - wr["rms_px"]) <= 1e-6 * max(1.0, wr["rms_px"])
    assert abs(gr["rms_init_px"] - wr["rms_init_px"]) <= 1e-6 * max(1.0, wr["rms_init_px"])


# ---- 3: a size equal to the call's size changes no byte

def with_call_size(rec):
    out = rec.copy()
    out["size"] = np.where(out["valid"] != 0, np.float32(TAG), 0)
    return out


def test_size_equal_to_the_call_size_changes_no_byte(gpu_detector):
    assert float(np.float32(TAG)) == TAG
    for name, obs, rec, dist, gate in LC.cpu_cases(K):
        if name not in ("exact", "mirrored", "gate", "dist5"):
            continue
        a = gpu_detector.localize(obs, rec, K, dist, TAG, max_tag_rms_px=gate, sigma_px=SIGMA)
        b = gpu_detector.localize(obs, with_call_size(rec), K, dist, TAG, max_tag_rms_px=gate, sigma_px=SIGMA)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), name
    import rig_cases as RC
    c = RC.case("side_by_side")
    a = c["rig"].localize(gpu_detector, c["obs"], c["rec"], TAG, 0.0, with_cov=True, sigma_px=SIGMA)
    b = c["rig"].localize(gpu_detector, c["obs"], with_call_size(c["rec"]), TAG, 0.0, with_cov=True, sigma_px=SIGMA)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    import smooth_cases as SC
    obs, rec, seed, dist = SC.shape(5, 4, 0)
    a = gpu_detector.smooth(obs, rec, K, dist, TAG, *SC.SHAPE_SIGMAS, max_iters=SC.COMPARE_ITERS, seed=seed)
    b = gpu_detector.smooth(obs, with_call_size(rec), K, dist, TAG, *SC.SHAPE_SIGMAS, max_iters=SC.COMPARE_ITERS, seed=seed)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_repeated_calls_on_a_sized_map_give_identical_bytes(gpu_detector):
    obs, rec, dist, _ = ZC.loc_case(65)
    first = None
    for _ in range(5):
        out, cov = localize_device(gpu_detector, obs, rec, dist, TAG, ZC.GATE, sigma_px=SIGMA)
        b = out.tobytes() + cov.tobytes()
        first = b if first is None else first
        assert b == first
    host = gpu_detector.localize(obs, rec, K, dist, TAG, max_tag_rms_px=ZC.GATE, sigma_px=SIGMA)
    assert host[0].tobytes() + host[1].tobytes() == first


# ---- 4: bad sizes

@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf], ids=["negative", "nan", "inf"])
def test_bad_size_is_an_unmapped_entry(gpu_detector, bad):
    """frame 0 sees tags 0 and 1, frame 4 (max_tags 2) only tag 16: with their sizes bad, frame 0 solves from tag 0 and frame 4
    has status 1, byte for byte what valid = 0 gives, in the host and the device form"""
    obs, rec, dist, _ = ZC.loc_case(2)
    a, b = rec.copy(), rec.copy()
    a["size"][[1, 16]] = bad
    b["valid"][[1, 16]] = 0
    got = gpu_detector.localize(obs, a, K, dist, TAG, sigma_px=SIGMA)
    want = gpu_detector.localize(obs, b, K, dist, TAG, sigma_px=SIGMA)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[0]["status"][4] == 1 and got[0]["status"][0] == 0 and got[0]["n_tags"][0] == 1 and got[0]["status"][1] == 2
    devf = localize_device(gpu_detector, obs, a, dist, TAG, sigma_px=SIGMA)
    assert devf[0].tobytes() == got[0].tobytes() and devf[1].tobytes() == got[1].tobytes()
    assert_loc_same(got[0], LR.localize(obs, a, K, dist, TAG), obs, a, dist)
    # the other solvers share the rule: the rig form and the sequence solve
    robs, rrec, rig = ZC.rig_case()
    a, b = rrec.copy(), rrec.copy()
    a["size"][[40, 43]] = bad
    b["valid"][[40, 43]] = 0
    assert rig.localize(gpu_detector, robs, a, TAG, 0.0).tobytes() == rig.localize(gpu_detector, robs, b, TAG, 0.0).tobytes()
    sobs, srec, seed = ZC.smooth_case()
    a, b = srec.copy(), srec.copy()
    a["size"][[37, 40]] = bad
    b["valid"][[37, 40]] = 0
    ga = gpu_detector.smooth(sobs, a, K, None, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed)
    gb = gpu_detector.smooth(sobs, b, K, None, TAG, *ZC.SMOOTH_SIGMAS, max_iters=ZC.SMOOTH_ITERS, seed=seed)
    assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()


# ---- 5: a uniform size on the map is the call's size

def test_uniform_size_is_the_call_size_on_the_device(gpu_detector):
    """test_sized_ref's uniform case with the records' poses from asl_solve_pnp_batch at s1 and at s2: the two descriptions of
    one scene give the same poses to the kernel-against-statement bar (not the same bytes: the scaled translation rounds
    differently)"""
    s1, s2 = 10.0, 25.0
    (a, rec_a), (b, rec_b) = ZC.uniform_case(s1, s2)
    for obs, size in ((a, s1), (b, s2)):
        _, _, T, ok = gpu_detector.solve_pnp(obs["corners"].reshape(-1, 4, 2), K, None, size)
        assert ok.all()
        obs["T"] = T[:, :3].reshape(obs.shape + (12,))
    got = gpu_detector.localize(a, rec_a, K, None, s1)
    want = gpu_detector.localize(b, rec_b, K, None, s2)
    worst = max(LC.rel_err(g["T"], w["T"]) for g, w in zip(got, want))
    print("uniform on the device: T rel_err %.3g, identical bytes: %s" % (worst, got.tobytes() == want.tobytes()))
    assert (got["status"] == 0).all() and (got["n_tags"] == 4).all() and np.array_equal(got["n_tags"], want["n_tags"])
    assert worst <= 1e-9, worst
    assert_loc_same(got, LR.localize(a, rec_a, K, None, s1), a, rec_a, None, tag_size=s1)


# ---- 6: end to end on rendered frames

E2E_W, E2E_H, E2E_FRAMES, E2E_RATIO = 641, 363, 16, 0.75
E2E_MARGIN = 2.0


def e2e_planes(tags, cams, ratios):
    """synth.render_planes for tags of several sizes: the renderer paints |X|, |Y| <= half of its one tag size, so a tag of
    ratio r is the plane whose tag coordinates are divided by r: rows 0 and 1 of its Hi times 1 / r = half / h_id.  The
    bounding boxes are those of the largest ratio (a box only bounds the pixels tested)."""
    planes, _ = synth.render_planes(E2E_W, E2E_H, tags, LC.TAG_OUTER * max([1.0] + list(ratios.values())), cams)
    Hi = planes["Hi"].reshape(planes.shape + (3, 3))
    for i, r in ratios.items():
        Hi[planes["tex"] == i, :2] /= r
    planes["Hi"] = Hi.reshape(planes["Hi"].shape)
    return planes


def e2e_run(det, tags, cams, ratios):
    """render -> detect + PnP at TAG -> pack -> localise against the map with the sizes of `ratios`, on one stream;
    (obs, map records, poses)"""
    import torch
    dev = torch.device("cuda:0")
    n, max_tags = len(cams), 8
    tm = TagMap.from_scene(tags)
    for i, r in ratios.items():
        tm.set_size(i, TAG * r)
    rec = tm.as_records()
    Kc = synth.camera_matrix(E2E_W, E2E_H, 45.0)
    planes = e2e_planes(tags, cams, ratios)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    d_tex, d_planes, d_map = torch.from_numpy(tex).to(dev), dev_bytes(planes, dev), dev_bytes(rec, dev)
    frames = torch.empty((n, E2E_H, E2E_W, 3), dtype=torch.uint8, device=dev)
    d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_out = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    det.render_frames_device(frames.data_ptr(), n, E2E_W, E2E_H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2], tex.shape[1],
                             0.5 * LC.TAG_OUTER, stream=st)
    det.submit_device(frames.data_ptr(), n, 3, E2E_W, E2E_H, stream=st, K=Kc, dist=np.zeros(4), tag_size=TAG)
    det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=st)
    det.localize_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), len(rec), d_out.data_ptr(), Kc, None, TAG, stream=st)
    torch.cuda.synchronize(dev)
    det.collect()
    return (d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, max_tags), rec, d_out.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n))


def e2e_errors(out, cams):
    truths = [LC.world_from_camera(p, r) for p, r in cams]
    rot = np.array([LC.rot_err(o["T"], t) for o, t in zip(out, truths)])
    tr = np.array([np.linalg.norm(o["T"][:3, 3] - t[:3, 3]) for o, t in zip(out, truths)])
    return float(np.sqrt(np.mean(rot ** 2))), float(np.sqrt(np.mean(tr ** 2)))


def test_end_to_end_with_two_tag_sizes():
    """16 rendered frames of 641 x 363 (the smallest the render tests use), 5 tags, ids 1 and 3 at 0.75 of the common size:
    render -> detect -> pack -> localise against the sized map.  The kernel is held to the statement on that block, and to the
    renderer's truth by: no worse than the same trajectory with all five tags at the common size, times E2E_MARGIN = 2.  The
    margin is reasoned, then measured: the detector's corner noise in pixels does not depend on the tag's size, and a tag at
    0.75 of the size holds the pose 0.75 times as firmly, so a scene of such tags alone would err by 1 / 0.75 = 1.33; the rest
    is for the scatter of a 16-frame RMS.  Measured on an MI355X: two sizes 0.470 mrad / 0.0463 units RMS, common size 0.497
    mrad / 0.0473, ratios 0.95 and 0.98; the statement with the sizes dropped from the map is off by 35 mrad / 3.4 units."""
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        rng = np.random.default_rng(2)                     # a scene whose tags stay 15 px inside the frame on these cameras
        tags = synth.random_scene(E2E_W, E2E_H, 5, rng)
        cams = [(tuple(rng.uniform(-1.5, 1.5, 3)), tuple(rng.uniform(-1, 1, 3))) for _ in range(E2E_FRAMES)]
        Kc = synth.camera_matrix(E2E_W, E2E_H, 45.0)
        obs, rec, out = e2e_run(det, tags, cams, {1: E2E_RATIO, 3: E2E_RATIO})
        obs0, rec0, out0 = e2e_run(det, tags, cams, {})
    finally:
        det.close()
    assert rec["size"].tolist() == [0, 7.5, 0, 7.5, 0] and not rec0["size"].any()
    assert (out["status"] == 0).all() and (out["n_tags"] >= 4).all() and (out0["n_tags"] >= 4).all()
    assert all(np.isin([1, 3], row["id"]).any() for row in obs)          # every frame sees a sized tag
    want = LR.localize(obs, rec, Kc, None, TAG)
    assert_loc_same(out, want, obs, rec, None, tol=1e-7, Kc=Kc)
    (rot, tr), (rot0, tr0) = e2e_errors(out, cams), e2e_errors(out0, cams)
    blind = e2e_errors(LR.localize(obs, ZC.without_sizes(rec), Kc, None, TAG), cams)
    print("two sizes: rot %.3g rad, trans %.3g; common size: rot %.3g rad, trans %.3g; ratios %.3g %.3g; sizes dropped: rot %.3g trans %.3g"
          % (rot, tr, rot0, tr0, rot / rot0, tr / tr0, blind[0], blind[1]))
    assert rot <= E2E_MARGIN * rot0 and tr <= E2E_MARGIN * tr0, (rot, rot0, tr, tr0)
