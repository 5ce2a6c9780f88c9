"""Camera calibration from tag observations: the NumPy statement (tests/calib_ref.py) on exact projections, with noise, on
degenerate input and on the distorted webcam through the CPU oracle detector; the calibration file and the board.  No GPU
needed."""
import os
import re

import numpy as np
import pytest

import calib_cases as CC
import calib_ref as CR
import localize_cases as LC
from aprilslam_amd import _lib, synth
from aprilslam_amd.calibrate import CALIB_RESULT_DTYPE, CalibrationResult
from aprilslam_amd.localize import TagMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def calibrate(obs, rec, **kw):
    return CR.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)


@pytest.mark.parametrize("target", ["scene", "board"])
def test_exact_projections_recover_the_camera(target):
    obs, rec, truths = CC.scene_case() if target == "scene" else CC.board_case()
    res, poses = calibrate(obs, rec, n_dist=5)
    assert res["status"] == 0 and res["n_frames_used"] == len(obs) and (poses["status"] == 0).all()
    assert np.abs(res["K"] - CC.K_TRUE).max() <= 1e-3, res["K"] - CC.K_TRUE
    assert CC.field_err(res["K"], res["dist"], CC.K_TRUE, CC.DIST5) <= 1e-3
    assert res["rms_px"] < 1e-3 and res["rms_init_px"] > 1.0      # float32 corners; the seed has no lens model
    for p, t in zip(poses, truths):
        assert LC.rel_err(p["T"], t) <= 1e-5 and LC.rot_err(p["T"], t) <= 1e-6
    assert (poses["rms_px"] < 1e-3).all() and (poses["rms_seed_px"] > poses["rms_px"]).all()


@pytest.mark.parametrize("n_dist", [0, 4, 5])
def test_coefficient_counts(n_dist):
    dist = {0: None, 4: CC.DIST4, 5: CC.DIST5}[n_dist]
    obs, rec, _ = CC.scene_case(dist=dist)
    res, _ = calibrate(obs, rec, n_dist=n_dist)
    assert res["status"] == 0 and np.abs(res["K"] - CC.K_TRUE).max() <= 1e-3
    assert CC.field_err(res["K"], res["dist"][:n_dist], CC.K_TRUE, dist) <= 1e-3
    assert (res["dist"][n_dist:] == 0).all() and (res["std"][4 + n_dist:] == 0).all() and (res["std"][:4 + n_dist] > 0).all()
    if n_dist:   # the model matters: a pinhole cannot fit the same corners
        assert calibrate(obs, rec, n_dist=0)[0]["rms_px"] > 0.1


def test_flags_hold_their_parameters():
    obs, rec, _ = CC.scene_case()
    K0 = CC.K_TRUE + np.array([[5.0, 0, 3.5], [0, -4.0, -2.25], [0, 0, 0]])
    res, _ = calibrate(obs, rec, n_dist=5, K_init=K0, flags=CR.FIX_PRINCIPAL_POINT)
    assert res["status"] == 0 and res["K"][0, 2] == K0[0, 2] and res["K"][1, 2] == K0[1, 2] and (res["std"][2:4] == 0).all()
    assert res["std"][0] > 0 and res["K"][0, 0] != K0[0, 0]
    res, _ = calibrate(obs, rec, n_dist=5, K_init=K0, flags=CR.FIX_ASPECT_RATIO)
    r = K0[0, 0] / K0[1, 1]
    assert res["status"] == 0 and res["K"][0, 0] == r * res["K"][1, 1] and res["std"][0] == 0 and res["std"][1] > 0
    bd, brec, _ = CC.board_case(dist=CC.DIST4)
    res, _ = calibrate(bd, brec, n_dist=4, flags=CR.ZERO_TANGENT_DIST)
    assert res["status"] == 0 and (res["dist"][2:] == 0).all() and (res["std"][6:] == 0).all() and (res["std"][4:6] > 0).all()
    # all three together, without K_init: the principal point stays the image centre, fx = fy
    res, _ = calibrate(obs, rec, n_dist=5, flags=7)
    assert res["status"] == 0 and res["K"][0, 2] == CC.W / 2 and res["K"][1, 2] == CC.H / 2 and res["K"][0, 0] == res["K"][1, 1]
    assert (res["std"][[0, 2, 3, 6, 7]] == 0).all()


def test_closed_form_alone():
    K = np.array([[905.0, 0.0, CC.W / 2], [0.0, 884.0, CC.H / 2], [0.0, 0.0, 1.0]])
    for obs, rec, _ in (CC.scene_case(K=K, dist=None), CC.board_case(K=K, dist=None)):
        frames = [(obs[f], CR.gather(obs[f], rec, LC.TAG_INNER)[0]) for f in range(len(obs))]
        fx, fy = CR.closed_form(frames, CC.W, CC.H, 0)
        assert abs(fx / 905.0 - 1) <= 1e-3 and abs(fy / 884.0 - 1) <= 1e-3, (fx, fy)
        f1, f2 = CR.closed_form(frames, CC.W, CC.H, CR.FIX_ASPECT_RATIO)
        assert f1 == f2 and 800.0 < f1 < 1000.0   # one focal length for both axes (the wrong model here): in range


def test_uncertainty_equals_the_dense_inverse():
    for obs, rec, _ in (CC.scene_case(), CC.board_case()):
        rng = np.random.default_rng(1)
        noisy = obs.copy()
        noisy["corners"] += rng.normal(0, 0.2, noisy["corners"].shape).astype(np.float32) * (noisy["id"] >= 0)[..., None]
        for kw in (dict(n_dist=5), dict(n_dist=4, flags=CR.FIX_ASPECT_RATIO | CR.ZERO_TANGENT_DIST)):
            res, poses = calibrate(noisy, rec, **kw)
            dense = CR.full_normal_std(noisy, rec, LC.TAG_INNER, res, poses, kw["n_dist"], kw.get("flags", 0))
            assert res["status"] == 0
            assert np.array_equal(dense == 0, res["std"] == 0)
            assert np.abs(dense - res["std"]).max() <= 1e-8 * np.abs(dense).max() * 10 and \
                np.allclose(res["std"], dense, rtol=1e-8, atol=0), (res["std"], dense)


def test_uncertainty_matches_the_spread_with_noise():
    """0.3 px of corner noise, 100 seeded trials: the empirical std of fx and cx is 0.7 - 1.4 times the reported one"""
    obs, rec, _ = CC.scene_case(n=6)
    rng = np.random.default_rng(2024)
    est, rep = [], []
    for _ in range(100):
        noisy = obs.copy()
        noisy["corners"] += rng.normal(0, 0.3, noisy["corners"].shape).astype(np.float32) * (noisy["id"] >= 0)[..., None]
        res, _ = calibrate(noisy, rec, n_dist=5, K_init=CC.K_TRUE, max_iters=12)
        assert res["status"] == 0
        est.append([res["K"][0, 0], res["K"][0, 2]])
        rep.append([res["std"][0], res["std"][2]])
    ratio = np.std(est, axis=0, ddof=1) / np.mean(rep, axis=0)
    assert ((ratio > 0.7) & (ratio < 1.4)).all(), ratio


def test_degenerate_input():
    bd, brec, truths = CC.board_case(n=6, fronto=True)
    res, poses = calibrate(bd, brec, n_dist=5)
    assert res["status"] == 2 and (poses["status"] == 4).all() and (res["K"] == 0).all()
    res, poses = calibrate(bd, brec, n_dist=5, K_init=CC.K_TRUE, flags=CR.FIX_PRINCIPAL_POINT)
    # fronto-parallel views leave focal length against depth undetermined: the solve runs, the fit is exact
    assert res["status"] == 0 and (poses["status"] == 0).all() and res["rms_px"] < 1e-3 and np.abs(res["K"] - CC.K_TRUE).max() <= 20
    for p, t in zip(poses, truths):
        assert LC.rot_err(p["T"], t) <= 1e-3
    for name, obs, rec, kw in CC.cpu_cases():
        if name == "one_tag":
            res, poses = calibrate(obs, rec, **kw)
            assert res["status"] == 1 and poses["status"][0] == 1 and poses["n_tags"][0] == 1
        if name == "padded":
            res, poses = calibrate(obs, rec, **kw)
            ref, rposes = calibrate(*CC.scene_case()[:2], n_dist=5)
            assert res.tobytes() == ref.tobytes()
            used = poses["status"] == 0
            assert list(np.flatnonzero(~used)) == [3, 8, 16] and (poses["status"][~used] == 1).all()
            assert poses[used].tobytes() == rposes.tobytes()


@pytest.fixture(scope="module")
def webcam_obs():
    """the distorted 640x480 webcam (test_gpu_render.py's lens) over a 3D scene of 12 tags, rendered on the host, through
    the CPU oracle detector"""
    import oracle_lib as O
    from aprilslam_amd.dist import pack_observations
    from aprilslam_amd.families import get_family
    tags, cams = webcam_scene(16)
    fam = get_family()
    obs = []
    for pos, rot in cams:
        frame, _ = synth.render_frame(CC.WEBCAM_W, CC.WEBCAM_H, tags, LC.TAG_OUTER, cam_position=pos, cam_rotation_deg=rot,
                                      fov_y_deg=CC.WEBCAM_FOV, dist=CC.WEBCAM_DIST)
        dets = [d for d in O.detect_bgr(frame, fam) if d["id"] < len(tags)]
        rec = np.zeros(len(dets), dtype=_lib.DET_DTYPE)
        rec["id"] = [d["id"] for d in dets]
        rec["corners"] = np.array([d["corners"] for d in dets]).reshape(-1, 4, 2)
        obs.append(pack_observations(rec, np.zeros(len(dets), dtype=_lib.POSE_DTYPE), [len(dets)], 16)[0])
    return np.stack(obs), TagMap.from_scene(tags).as_records(), cams


def webcam_scene(n, seed=11):
    rng = np.random.default_rng(seed)
    tags = synth.random_scene(CC.WEBCAM_W, CC.WEBCAM_H, 12, rng, fov_y_deg=CC.WEBCAM_FOV)
    cams = [(tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-4, 4, 3))) for _ in range(n)]
    return tags, cams


def test_detector_corners_of_the_distorted_webcam(webcam_obs):
    """Measured: fx +0.039 %, fy +0.034 %, cx -0.03 px, cy +0.08 px, distortion field 0.18 px at worst over the image
    (16 x 16 grid), final RMS 0.18 px (5.5 px after the seed, which has no lens model), camera rotation 0.56 mrad at worst; 16 frames of
    9-12 tags, 8 iterations.  The detector's corners sit on straight-line fits of slightly curved edges."""
    obs, rec, cams = webcam_obs
    K = synth.camera_matrix(CC.WEBCAM_W, CC.WEBCAM_H, CC.WEBCAM_FOV)
    res, poses = CR.calibrate(obs, rec, LC.TAG_INNER, CC.WEBCAM_W, CC.WEBCAM_H, n_dist=5)
    assert res["status"] == 0 and res["n_frames_used"] == len(obs)
    e = np.abs(res["K"] - K)
    assert e[0, 0] / K[0, 0] <= 2e-3 and e[1, 1] / K[1, 1] <= 2e-3 and e[0, 2] <= 1.5 and e[1, 2] <= 1.5, res["K"]
    assert CC.field_err(res["K"], res["dist"], K, CC.WEBCAM_DIST, CC.WEBCAM_W, CC.WEBCAM_H) <= 0.5
    assert res["rms_px"] < 0.3
    for p, (pos, rot) in zip(poses, cams):
        assert LC.rot_err(p["T"], LC.world_from_camera(pos, rot)) <= 3e-3


def test_calibration_file_round_trip(tmp_path):
    from aprilslam_amd.video_detection import load_camera_calibration
    obs, rec, truths = CC.board_case(dist=CC.DIST4)
    res, poses = calibrate(obs, rec, n_dist=4)
    cr = CalibrationResult(res, poses, 4)
    assert cr.ok and cr.camera_params["dist_coeffs"].shape == (4, 1) and np.array_equal(cr.camera_params["camera_matrix"], res["K"])
    path = str(tmp_path / "camera_calibration_parameters.npz")
    cr.save_npz(path)
    got = load_camera_calibration(path)
    assert np.array_equal(got["camera_matrix"], res["K"]) and np.array_equal(got["dist_coeffs"].ravel(), res["dist"][:4])
    with np.load(path) as z:
        assert sorted(z.files) == ["camera_matrix", "dist_coeffs", "rvecs", "tvecs"]
        rv, tv = z["rvecs"], z["tvecs"]
    assert rv.shape == (len(obs), 3, 1) and tv.shape == (len(obs), 3, 1)
    from aprilslam_amd.tag_detector import rodrigues
    for r, t, T in zip(rv, tv, truths):
        Tcw = np.linalg.inv(T)
        assert np.abs(rodrigues(r) - Tcw[:3, :3]).max() <= 1e-5 and np.abs(t.ravel() - Tcw[:3, 3]).max() <= 1e-3


def test_grid_board_equals_the_synth_scene():
    a = TagMap.grid(CC.BOARD_ROWS, CC.BOARD_COLS, LC.TAG_INNER, CC.BOARD_SPACING)
    b = TagMap.from_scene(CC.board_scene())
    assert a.ids() == b.ids() == list(range(CC.BOARD_ROWS * CC.BOARD_COLS))
    assert a.as_records().tobytes() == b.as_records().tobytes()
    g = TagMap.grid(2, 3, 1.0, 2.5, first_id=10)
    assert g.ids() == list(range(10, 16)) and np.array_equal(g[14][:3, 3], [2.5, 2.5, 0.0])
    for bad in (dict(rows=0), dict(spacing=0.5), dict(first_id=-1)):
        with pytest.raises(ValueError):
            TagMap.grid(**{**dict(rows=2, cols=2, tag_size=1.0, spacing=2.0), **bad})


def test_calib_result_dtype_matches_the_header():
    assert CALIB_RESULT_DTYPE.itemsize == 216
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    assert re.search(r"\} asl_calib_result;\s*/\* 216 bytes", src)
    for name in ("asl_calibrate_frames_device", "asl_calibrate_batch"):
        assert name in _lib.EXPORTS
    for flag, v in (("FIX_PRINCIPAL_POINT", 1), ("FIX_ASPECT_RATIO", 2), ("ZERO_TANGENT_DIST", 4)):
        assert re.search(r"#define ASL_CALIB_%s\s+%d\b" % (flag, v), src) and getattr(CR, flag) == v
