"""The NumPy statement of the rig mounting calibration (tests/rig_calib_ref.py) against the truth the inputs were made
with, and its Schur route against a dense inverse of the full normal matrix.  CPU only: the statement is what the kernels
are compared with (tests/test_gpu_rig_calib.py), so it is checked on its own here."""
import numpy as np
import pytest

import pose_cov_ref as PC
import rig_calib_cases as CC
import rig_calib_ref as CR
from solver_checks import assert_cov_close

EXACT_ROT_DEG, EXACT_TRANS = 1e-4, 1e-4     # the floor is the float32 corners; the statement's own worst is in the docstring below
SIGMA = 0.5


@pytest.fixture(scope="module")
def solved():
    """calibrate() of every case once, sigma_px given: {name: (case, rig_out, result, cov, poses, details)}"""
    out = {}
    for name in CC.NAMES:
        c = CC.case(name)
        det = {}
        out[name] = (c,) + CR.calibrate(c["obs"], c["rec"], c["rig0"], c["tag_size"], sigma_px=SIGMA, details=det) + (det,)
    return out


def worst_error(rig_out, truth, cams):
    e = [CR.mounting_error(rig_out["E"][k], truth.cameras[k].T_cam_rig) for k in cams]
    return max(x[0] for x in e), max(x[1] for x in e)


@pytest.mark.parametrize("name", CC.EXACT)
def test_exact_corners_return_the_true_mountings(solved, name):
    """Mountings off by 2 degrees and 0.5 units, exact corners (float32).  The statement's own worst errors:
    pair 2.1e-6 deg 4.4e-6 units, mixed < 1e-6 deg 1.1e-6 units, ring8 1.7e-6 deg 6.1e-6 units, dropout 1.7e-6 deg 4.1e-6
    units; every case starts at rms 9 to 23 px and ends at 2e-5 px."""
    c, out, res, cov, poses, _ = solved[name]
    n = len(out)
    rot0, tr0 = worst_error(c["rig0"].as_records(), c["truth"], range(1, n))
    rot, tr = worst_error(out, c["truth"], range(1, n))
    print(name, "initial %.3f deg %.3f units, final %.2e deg %.2e units, rms %.3g -> %.3g px, %d trials"
          % (rot0, tr0, rot, tr, res["rms_init_px"], res["rms_px"], res["iterations"]))
    assert res["status"] == 0 and res["n_solved"] == n - 1
    assert list(res["cam_status"][:n]) == [1] + [0] * (n - 1) and not res["cam_status"][n:].any()
    assert rot0 > 1.9 and rot <= EXACT_ROT_DEG and tr <= EXACT_TRANS
    assert out["E"][0].tobytes() == c["rig0"].as_records()["E"][0].tobytes()           # the gauge
    for f in ("K", "dist", "n_dist"):
        assert out[f].tobytes() == c["rig0"].as_records()[f].tobytes()
    assert res["rms_px"] < 1e-3 < res["rms_init_px"]
    assert list(cov["status"]) == [1] + [0] * (n - 1) and (cov["sigma_px"] == SIGMA).all()
    used = poses["status"] == 0
    assert res["n_frames_used"] == used.sum() and res["n_corners"] == 4 * poses["n_tags"][used].sum()
    assert (cov["dof"][1:] == 2 * res["n_corners"] - 6 * res["n_frames_used"] - 6 * res["n_solved"]).all()


def test_dropout_frames_stay_outside(solved):
    """camera 1 has no slot in frames 2 and 3: one camera is no constraint on a mounting, the frames keep their seed's record"""
    c, out, res, cov, poses, det = solved["dropout"]
    assert list(poses["status"]) == [0, 0, 5, 5, 0, 0] and list(res["cam_frames"][:2]) == [4, 4]
    for f in (2, 3):
        want = det["seed"][f].copy()
        want["status"] = 5
        assert poses[f].tobytes() == want.tobytes()


@pytest.mark.parametrize("seed", range(5))
def test_one_small_tag_per_camera(seed):
    """The case the feature exists for: two cameras back to back, each seeing one small tag of its own, corners noisy by
    0.3 px; the averaged single-camera mounting is poisoned by mirrored poses.  The statement over seeds 0..4:
        averaged   21.45 / 20.12 / 20.59 / 20.20 / 19.95 degrees, 79.26 / 74.29 / 74.89 / 74.91 / 74.97 units
        joint       0.160 / 0.386 / 0.097 / 0.420 / 0.121 degrees, 0.246 / 0.419 / 0.296 / 0.309 / 0.500 units
        worst |error| / std over the 6 components: 0.68 / 1.92 / 0.51 / 1.46 / 1.21; 21 to 23 trials, rms 0.30 to 0.35 px
    The bound (rig_calib_cases.ONE_TAG_ROT_DEG, ONE_TAG_TRANS) is twice the worst of those."""
    c = CC.one_tag(seed)
    out, res, cov, poses = CR.calibrate(c["obs"], c["rec"], c["rig0"], c["tag_size"])
    T = c["truth"].cameras[1].T_cam_rig
    rot0, tr0 = CR.mounting_error(c["rig0"].cameras[1].T_cam_rig[:3], T)
    rot, tr = CR.mounting_error(out["E"][1], T)
    err = PC.pose_error(out["E"][1][:, :3], out["E"][1][:, 3], T[:3, :3], T[:3, 3])
    std = np.sqrt(np.diag(cov["cov"][1]))
    print("seed %d: averaged %.2f deg %.2f units, joint %.4f deg %.4f units, %d trials, rms %.4f px, sigma %.4f, worst |error| / std %.2f"
          % (seed, rot0, tr0, rot, tr, res["iterations"], res["rms_px"], res["sigma_px"], np.abs(err / std).max()))
    assert res["status"] == 0 and res["n_frames_used"] == 24 and res["iterations"] < 30
    assert rot0 > 10.0
    assert rot <= CC.ONE_TAG_ROT_DEG and tr <= CC.ONE_TAG_TRANS
    assert (np.abs(err) <= 4 * std).all()
    assert cov["status"][1] == 0 and 0.2 < res["sigma_px"] < 0.4 and cov["sigma_px"][1] == res["sigma_px"]


@pytest.mark.parametrize("name", CC.EXACT + ["one_tag", "island"])
def test_schur_route_equals_the_dense_inverse(solved, name):
    c, out, res, cov, poses, _ = solved[name]
    full, H = CR.full_normal_cov(c["obs"], c["rec"], out, c["tag_size"], res, poses, SIGMA)
    assert sorted(full) == [k for k in range(len(out)) if cov["status"][k] == 0]
    for k, ref in full.items():
        assert_cov_close(cov["cov"][k], ref, H, (name, k))
    # and through the statement's own re-linearisation at the solution
    again, S = CR.schur_cov(c["obs"], c["rec"], out, c["tag_size"], res, poses, SIGMA)
    for k, ref in again.items():
        assert_cov_close(cov["cov"][k], ref, S, (name, k))


def test_a_camera_that_shares_no_frame_is_held(solved):
    c, out, res, cov, poses, _ = solved["island"]
    rig0 = c["rig0"].as_records()
    assert res["status"] == 0 and res["n_solved"] == 1
    assert list(res["cam_status"][:3]) == [1, 0, 2] and list(res["cam_frames"][:3]) == [6, 6, 0]
    assert out["E"][2].tobytes() == rig0["E"][2].tobytes() and out["E"][0].tobytes() == rig0["E"][0].tobytes()
    assert list(cov["status"]) == [1, 0, 1] and not cov["cov"][2].any() and cov["dof"][2] == 0
    # the two connected cameras solve as the pair alone does
    pair = solved["pair"]
    assert worst_error(out, c["truth"], [1])[0] <= EXACT_ROT_DEG and pair[2]["n_corners"] == res["n_corners"]


def test_nothing_to_solve(solved):
    c, out, res, cov, poses, det = solved["nothing"]
    assert res["status"] == 1 and res["n_solved"] == 0 and res["n_frames_used"] == 0 and res["iterations"] == 0
    assert out.tobytes() == c["rig0"].as_records().tobytes()
    assert (poses["status"] == 5).all() and (cov["status"] == 1).all() and not cov["cov"].any()
    assert np.array_equal(poses["T"], det["seed"]["T"])


def test_result_round_trips_through_save_and_load(solved, tmp_path):
    """RigCalibrationResult.save / load on the statement's output, with and without the .npz suffix"""
    from aprilslam_amd.rig import Rig, RigCalibrationResult
    c, out, res, cov, poses, _ = solved["island"]
    r = RigCalibrationResult(Rig.from_records(out), res, cov, poses)
    assert r.ok and r.mounting_std().shape == (3, 6) and not r.mounting_std()[[0, 2]].any() and (r.mounting_std()[1] > 0).all()
    for name in ("cal", "cal2.npz"):
        r.save(str(tmp_path / name))
        q = RigCalibrationResult.load(str(tmp_path / name))
        assert q.rig.as_records().tobytes() == out.tobytes() and q.result.tobytes() == res.tobytes() and q.result.shape == ()
        assert q.cov.tobytes() == cov.tobytes() and q.poses.tobytes() == poses.tobytes() and q.ok
        assert Rig.load(str(tmp_path / name.replace(".npz", "")) + ".npz").as_records().tobytes() == out.tobytes()
    assert sorted(f.name for f in tmp_path.iterdir()) == ["cal.npz", "cal.records.npz", "cal2.npz", "cal2.records.npz"]


def test_the_sweeps_reach_through_a_chain():
    """0-1 share a frame late, 1-2 one early: camera 2 joins in the second sweep; 3 and 4 share frames among themselves only"""
    masks = [{1, 2}, {3, 4}, {0}, {0, 1}, {2}, set()]
    reach, used = CR.connect(masks, 5)
    assert reach == {0, 1, 2} and used == [0, 3]


def test_list_sum_order():
    rows = np.arange(40, dtype=np.float64).reshape(20, 2)
    assert np.array_equal(CR.list_sum(rows), rows.sum(axis=0))
    x = np.array([[1e16], [1.0], [1.0], [-1e16]])             # chunks of one: ((1e16 + 1) + 1) - 1e16 in order
    assert CR.list_sum(x)[0] == 0.0
