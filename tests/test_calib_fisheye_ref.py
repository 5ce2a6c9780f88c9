"""The NumPy statement of the fisheye calibration (tests/calib_fisheye_ref.py) on the CPU: its projection against
rectify.project_rays, its Jacobians against central differences, the focal ladder, the recovery of a known lens, the std
route, the recorded bounds of tests/calib_fisheye_cases.py, and the library's new entry points."""
import numpy as np
import pytest

import calib_fisheye_cases as FC
import calib_fisheye_ref as FR
import calib_ref as CR
import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import _lib, rectify
from aprilslam_amd.calibrate import CalibrationResult


@pytest.fixture(scope="module")
def solved():
    """{case: (record, poses, trace)} of the statement, each case solved once"""
    out = {}

    def get(name):
        if name not in out:
            _, obs, rec, kw = FC.case(name)
            trace = {}
            out[name] = FR.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, trace=trace, **kw) + (trace,)
        return out[name]
    return get


def random_rays(n, max_deg, seed):
    rng = np.random.default_rng(seed)
    th, ph = np.radians(rng.uniform(0.0, max_deg, n)), rng.uniform(0.0, 2 * np.pi, n)
    return rng.uniform(5.0, 80.0, n)[:, None] * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)


def test_entry_points_and_the_model_argument_exist():
    import inspect
    assert "asl_calibrate_lens_frames_device" in _lib.EXPORTS and "asl_calibrate_lens_batch" in _lib.EXPORTS
    assert "model" in inspect.signature(_lib.Detector.calibrate).parameters
    assert "model" in inspect.signature(_lib.Detector.calibrate_device).parameters
    L = _lib.load()
    assert len(L.asl_calibrate_lens_batch.argtypes) == len(L.asl_calibrate_batch.argtypes) + 1


def test_projection_is_rectify_project_rays():
    P = random_rays(2000, 170.0, 1)
    got = FR.project(FR.camera(FC.K_TRUE, FC.DIST), P)
    want = rectify.project_rays(P, FC.K_TRUE, FC.DIST, "fisheye")
    # the two differ by the arctangent alone (atan2_pos against np.arctan2: 2 ulp of theta <= pi), times f (1 + sum |k| i theta^2i)
    assert np.abs(got - want).max() <= 1e-11


def test_jacobians_match_central_differences():
    cam = FR.camera(FC.K_TRUE, FC.DIST)
    P = random_rays(200, 170.0, 2)
    _, J = FR.project(cam, P, jac=True)
    h = 1e-5
    for a in range(3):
        d = np.zeros(3)
        d[a] = h
        num = (FR.project(cam, P + d) - FR.project(cam, P - d)) / (2 * h)
        assert np.abs(J[:, :, a] - num).max() <= 1e-6 * max(1.0, np.abs(num).max()), a
    # pose, intrinsics and coefficients: the rows of linearise against differences of the residuals
    _, obs, rec, _ = FC.case("board4")
    _, Xw, uv = CR.gather(obs[0], rec, LC.TAG_INNER)
    R, t = FC.board_block()[2][0]
    theta = np.array([FC.K_TRUE[0, 0], FC.K_TRUE[1, 1], FC.K_TRUE[0, 2], FC.K_TRUE[1, 2]] + list(FC.DIST) + [0.0])

    def resid(th, R_, t_):
        return (FR.project(tuple(th[:8]), Xw @ R_.T + t_) - uv).reshape(-1)

    cost, H, g = FR.linearise(theta, R, t, Xw, uv, 4, 0, 1.0)
    cols = []
    for a in range(6):
        d = np.zeros(6)
        d[a] = 1e-6
        Rp, Rm = LR.rodrigues(d[:3]), LR.rodrigues(-d[:3])
        cols.append((resid(theta, Rp @ R, Rp @ t + d[3:]) - resid(theta, Rm @ R, Rm @ t - d[3:])) / 2e-6)
    for a in range(8):
        d = np.zeros(9)
        d[a] = 1e-6
        cols.append((resid(theta + d, R, t) - resid(theta - d, R, t)) / 2e-6)
    J = np.stack(cols, axis=1)
    Hn, gn = J.T @ J, J.T @ resid(theta, R, t)
    assert np.abs(H[:14, :14] - Hn).max() <= 1e-6 * np.abs(Hn).max()
    assert np.abs(g[:14] - gn).max() <= 1e-6 * max(1.0, np.abs(gn).max())
    assert not H[14].any() and not H[:, 14].any() and abs(cost - resid(theta, R, t) @ resid(theta, R, t)) <= 1e-9 * max(cost, 1e-30)


def test_the_axis_is_the_finite_limit():
    cam = FR.camera(FC.K_TRUE, FC.DIST)
    P = np.array([[0.0, 0.0, 40.0], [1e-9, -2e-9, 40.0]])
    uv, J = FR.project(cam, P, jac=True)
    assert np.array_equal(uv[0], [FC.K_TRUE[0, 2], FC.K_TRUE[1, 2]])
    want = np.array([[FC.K_TRUE[0, 0] / 40.0, 0.0, 0.0], [0.0, FC.K_TRUE[1, 1] / 40.0, 0.0]])
    assert np.array_equal(J[0], want) and np.all(np.isfinite(J))
    assert np.abs(J[1] - want).max() <= 1e-9          # and the limit is the neighbourhood's value
    # the case that has such a corner: its camera point is exactly on the axis, its pixel exactly the principal point
    _, obs, rec, _ = FC.case("on_axis")
    Ra, ta = FC.on_axis_frame(rec)
    _, Xw, uv_o = CR.gather(obs[-1], rec, LC.TAG_INNER)
    Pc = Xw @ Ra.T + ta
    k = int(np.argmin(np.hypot(Pc[:, 0], Pc[:, 1])))
    assert Pc[k, 0] == 0.0 and Pc[k, 1] == 0.0 and Pc[k, 2] == 40.0
    assert np.array_equal(uv_o[k], [FC.K_TRUE[0, 2], FC.K_TRUE[1, 2]])
    c, H, g = FR.linearise(np.array(list(cam) + [0.0]), Ra, ta, Xw, uv_o, 4, 0, 1.0)
    assert np.isfinite(c) and np.all(np.isfinite(H)) and np.all(np.isfinite(g))


def test_a_corner_past_90_degrees_is_an_ordinary_corner():
    cam = FR.camera(FC.K_TRUE, FC.DIST)
    X = np.array([[30.0, 2.0, -3.0], [0.0, 0.0, 0.0]])      # 96 degrees off axis; and the camera centre itself
    uv = FR.project(cam, X[:1])
    e = FR.corner_costs(cam, np.eye(3), np.zeros(3), X, np.r_[uv, [[0.0, 0.0]]])
    assert e[0] == 0.0 and e[1] == LR.BEHIND_COST


def test_conditions_on_the_inputs():
    obs, rec, poses = FC.board_block()
    assert ((obs["flags"] & 1).sum(axis=1) >= 25).all()
    assert FC.off_axis_deg(obs, rec, poses).max() > 90.0
    with pytest.raises(ValueError):
        FR.free_params(4, FR.ZERO_TANGENT_DIST)
    with pytest.raises(ValueError):
        FR.free_params(5, 0)


def test_ladder_has_one_clean_minimum(solved):
    _, _, trace = solved("board4")
    s, j = trace["scores"], trace["rung"]
    assert len(s) == FR.N_RUNGS and 0 < j < FR.N_RUNGS - 1
    assert all(s[k] > s[k + 1] for k in range(j)) and all(s[k] < s[k + 1] for k in range(j, FR.N_RUNGS - 1))
    f = [FR.rung_focal(k, FC.W, FC.H) for k in range(FR.N_RUNGS)]
    assert f[4] == max(FC.W, FC.H) / np.pi and np.allclose(np.array(f[1:]) / np.array(f[:-1]), 2 ** 0.25, rtol=1e-15)
    assert f[j] / 2 ** 0.125 <= 0.5 * (FC.K_TRUE[0, 0] + FC.K_TRUE[1, 1]) <= f[j] * 2 ** 0.125


@pytest.mark.parametrize("name", ["board4", "board0", "k_init", "on_axis"])
def test_recovers_the_lens_from_exact_corners(solved, name):
    res, poses, _ = solved(name)
    assert res["status"] == 0 and res["n_frames_used"] == len(poses) and (poses["status"] == 0).all()
    f, c, fld = FC.lens_errors(res, dist=None if name == "board0" else FC.DIST)
    print(name, f, c, fld, res["rms_px"])
    assert f <= 1e-3 / FC.K_TRUE[0, 0] and c <= 1e-3 and fld <= 1e-3     # 1e-3 px-equivalent, each
    truth = FC.board_block()[2]
    for p, (R, t) in zip(poses[:6], truth):
        assert LC.rel_err(p["T"], FC.world_from_camera(R, t)) <= 1e-6
    assert res["dist"][4] == 0 and res["std"][8] == 0
    if name == "board0":
        assert not res["dist"].any() and not res["std"][4:].any()


def test_statuses_flags_and_frames_that_do_not_take_part(solved):
    b4, bp, _ = solved("board4")
    res, poses, _ = solved("padded")
    assert np.array_equal(poses["status"], [0, 1, 0, 0, 1, 0, 0, 1, 0]) and res.tobytes() == b4.tobytes()
    assert poses[[0, 2, 3, 5, 6, 8]].tobytes() == bp.tobytes()
    res, poses, _ = solved("one_tag")
    assert res["status"] == 1 and poses["status"][0] == 1
    res, _, _ = solved("fix_pp")
    assert res["status"] == 0 and res["K"][0, 2] == FC.K_INIT_NEAR[0, 2] and res["K"][1, 2] == FC.K_INIT_NEAR[1, 2] and not res["std"][2:4].any()
    res, _, _ = solved("fix_aspect")
    assert res["status"] == 0 and res["K"][0, 0] == res["K"][1, 1] and res["std"][0] == 0


def test_far_only_frame_is_dropped_and_changes_nothing_else(solved):
    _, obs, rec, kw = FC.case("far_only")
    res, poses, _ = solved("far_only")
    assert (obs["flags"][3] & 1).sum() >= 2 and poses["status"][3] == 3 and poses["seed_slot"][3] == -1
    without = np.delete(obs, 3, axis=0)
    r2, p2 = FR.calibrate(without, rec, LC.TAG_INNER, FC.W, FC.H, **kw)
    assert res.tobytes() == r2.tobytes() and np.delete(poses, 3).tobytes() == p2.tobytes()


def test_std_of_the_schur_route_is_the_full_inverse(solved):
    for name, n_dist, flags in (("board4", 4, 0), ("fix_aspect", 4, FR.FIX_ASPECT_RATIO)):
        _, obs, rec, _ = FC.case(name)
        res, poses, _ = solved(name)
        full = FR.full_normal_std(obs, rec, LC.TAG_INNER, res, poses, n_dist, flags)
        assert np.array_equal(full == 0, res["std"] == 0)
        assert np.abs(full - res["std"]).max() <= 1e-6 * np.abs(res["std"]).max()


def test_noisy_corners_hold_the_recorded_bounds():
    f, c, fld = FC.measure_noisy()
    rec = FC.recorded()
    print("noisy", f, c, fld)
    for got, key in ((f, "noisy_f_rel"), (c, "noisy_c_px"), (fld, "noisy_field_px")):
        assert rec[key][0] > 0 and got <= rec[key][1], (key, got, rec[key])


def test_end_to_end_scene_holds_the_recorded_bounds():
    (f, c, fld), res, poses, obs = FC.measure_e2e()
    assert FC.e2e_frames().shape == (6, FC.H, FC.W, 3) and obs.shape[1] <= 12
    assert ((obs["flags"] & 1).sum(axis=1) >= 2).all()                      # the oracle finds >= 2 board tags in every frame
    assert res["n_frames_used"] == len(obs) and (poses["status"] == 0).all()   # and every frame is used
    rec = FC.recorded()
    print("e2e", f, c, fld, res["rms_px"])
    for got, key in ((f, "e2e_f_rel"), (c, "e2e_c_px"), (fld, "e2e_field_px")):
        assert rec[key][0] > 0 and got <= rec[key][1], (key, got, rec[key])


def test_result_carries_the_lens(tmp_path, solved):
    from aprilslam_amd.video_detection import load_camera_calibration
    res, poses, _ = solved("board4")
    cr = CalibrationResult(res, poses, 4, "fisheye")
    assert cr.lens_model == "fisheye" and cr.camera_params["lens_model"] == "fisheye" and cr.camera_params["dist_coeffs"].shape == (4, 1)
    assert CalibrationResult(res, poses, 4).camera_params["lens_model"] == "brown"
    path = str(tmp_path / "fisheye.npz")
    cr.save_npz(path)
    got = load_camera_calibration(path)
    assert got["lens_model"] == "fisheye" and np.array_equal(got["camera_matrix"], cr.K) and np.array_equal(got["dist_coeffs"].ravel(), cr.dist)
    vs = cr.view_set(3, 90, (640, 480))
    assert len(vs) == 3 and vs.model == rectify.LENS_FISHEYE and np.array_equal(vs.K, cr.K) and np.array_equal(vs.dist, cr.dist)
    with pytest.raises(ValueError):
        CalibrationResult(res, poses, 4, "pinhole")
