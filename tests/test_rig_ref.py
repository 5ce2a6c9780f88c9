"""Rig localisation: the NumPy statement (tests/rig_ref.py) against the truth of exact projections, against the
single-camera statement (tests/localize_ref.py) it must reduce to, against a change of the rig frame, and against what it
is for: a rig pose better than any one camera's, with an honest covariance.  Rig.from_camera_poses and the container.
No GPU needed."""
import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
import pose_cov_ref as PC
import rig_cases as RC
import rig_ref as RR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE
from aprilslam_amd.rig import Rig, RigCamera

K = synth.camera_matrix(LC.W, LC.H, 45.0)

NOISE_PX = 0.3
N_DRAWS = 200
N_COV = 500
COV_BOUND = 5 * np.sqrt(12.0 / N_COV)    # chi-square(6): variance 12; five standard errors of the mean of N_COV


@pytest.mark.parametrize("name", RC.NAMES)
def test_exact_projections_recover_the_rig_pose(name):
    """the bar of test_localize_ref.test_exact_corners_recover_the_pose for records (float32 corners): 1e-5, rms < 1e-3 px"""
    c = RC.case(name)
    out = RR.localize(c["obs"], c["rec"], c["rig"], c["tag_size"], c["gate"])
    part = ((c["obs"]["flags"] & 1) != 0).sum(axis=(0, 2))
    for f, (o, truth) in enumerate(zip(out, c["truth"])):
        assert o["status"] == 0 and o["n_tags"] + o["n_rejected"] == part[f], (name, f)
        assert LC.rel_err(o["T"], truth) <= 1e-5 and o["rms_px"] < 1e-3, (name, f, LC.rel_err(o["T"], truth), o["rms_px"])
        assert 0 <= o["seed_slot"] % LR.MIRRORED < c["obs"].shape[0] * c["obs"].shape[2]
    if name == "gate":
        assert (out["n_rejected"] == 2).all()        # the moved tag, once per camera
    else:
        assert (out["n_rejected"] == 0).all()
    if name == "mirror_all":
        assert (out["seed_slot"] >= LR.MIRRORED).all()
    if name == "one_seeder":
        assert (out["seed_slot"] % LR.MIRRORED == c["obs"].shape[2]).all()      # camera 1's slot 0, the only one with a pose
    if name == "back_to_back":
        assert ((c["obs"]["flags"] & 1) != 0).sum(axis=2).max() <= 2
    if name == "slots_256":
        assert c["obs"].shape[0] * c["obs"].shape[2] == 256


def test_statuses_without_tags_or_seeds():
    c = RC.case("side_by_side")
    obs = c["obs"].copy()
    obs["flags"][:, 0] = 0            # frame 0: no slot taking part in any camera -> status 1
    obs["flags"][:, 1] &= 1           # frame 1: nothing with a PnP in any camera -> status 2
    out, cov = RR.localize(obs, c["rec"], c["rig"], c["tag_size"], 0.0, sigma_px=0.5)
    assert list(out["status"][:3]) == [1, 2, 0]
    for f in (0, 1):
        assert np.array_equal(out["T"][f], np.eye(4)) and out["n_tags"][f] == 0 and out["seed_slot"][f] == -1
        assert cov["status"][f] == 1 and cov["dof"][f] == 0 and cov["sigma_px"][f] == 0.5 and not cov["cov"][f].any()


@pytest.mark.parametrize("case", [c[0] for c in LC.cpu_cases(K)])
def test_one_camera_at_the_identity_is_the_single_camera_statement(case):
    name, obs, rec, dist, gate = [c for c in LC.cpu_cases(K) if c[0] == case][0]
    want = LR.localize(obs, rec, K, dist, LC.TAG_INNER, gate)
    got = RR.localize(obs[None], rec, Rig([RigCamera(K, dist, np.eye(4))]), LC.TAG_INNER, gate)
    for f, (g, w) in enumerate(zip(got, want)):
        for field in ("status", "n_tags", "n_rejected", "seed_slot"):
            assert g[field] == w[field], (f, field)
        assert LC.rel_err(g["T"], w["T"]) <= 1e-12, (f, LC.rel_err(g["T"], w["T"]))
        assert abs(g["rms_px"] - w["rms_px"]) <= 1e-12 * max(1.0, w["rms_px"])
        assert abs(g["rms_seed_px"] - w["rms_seed_px"]) <= 1e-12 * max(1.0, w["rms_seed_px"])


@pytest.mark.parametrize("name", ["side_by_side", "back_to_back", "mixed_models", "gate"])
def test_moving_the_rig_frame_moves_the_result(name):
    """E_c -> E_c inv(D) describes the same rig in a frame moved by D: world<-rig -> world<-rig inv(D)"""
    c = RC.case(name)
    D = RC.transform((0.3, -0.5, 0.2), (3.0, -1.5, 2.0))
    Di = np.linalg.inv(D)
    moved = Rig([RigCamera(rc.K, rc.dist, rc.T_cam_rig @ Di) for rc in c["rig"].cameras])
    a = RR.localize(c["obs"], c["rec"], c["rig"], c["tag_size"], c["gate"])
    b = RR.localize(c["obs"], c["rec"], moved, c["tag_size"], c["gate"])
    for f, (x, y) in enumerate(zip(a, b)):
        for field in ("status", "n_tags", "n_rejected", "seed_slot"):
            assert x[field] == y[field], (f, field)
        assert LC.rel_err(y["T"], x["T"] @ Di) <= 1e-9, (f, LC.rel_err(y["T"], x["T"] @ Di))


def add_noise(obs, rng, sigma):
    out = obs.copy()
    out["corners"] = (obs["corners"].astype(np.float64) + rng.normal(scale=sigma, size=obs["corners"].shape)).astype(np.float32)
    return out


def test_the_rig_beats_each_of_its_cameras():
    """Back to back, two tags of side 10 at about 120 units (about 72 px across) in front of each camera, Gaussian corner
    noise of 0.3 px, 200 draws on frame 0.  Each camera alone is localised with the single-camera statement
    (localize_ref.localize) and composed with the true mounting.  RMS error of world<-rig against the truth, observed:

        rig        rotation 0.351 mrad, translation 0.0425 units
        camera 0   rotation 9.266 mrad, translation 1.1264 units
        camera 1   rotation 6.839 mrad, translation 0.8542 units

    Two tags side by side leave one camera's tilt about the line through them weak; the other camera's pair, seen through
    the known mounting, pins it.  Only the strict inequality is asserted."""
    tm, rig, poses = RC.back_to_back()
    rec = tm.as_records()
    obs = RC.exact_block(tm, rig, poses[:1], LC.TAG_INNER, 4)
    truth = poses[0]
    rng = np.random.default_rng(404)
    err = {"rig": [], 0: [], 1: []}

    def pose_err(T):
        return LC.rot_err(T, truth), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))

    for _ in range(N_DRAWS):
        noisy = add_noise(obs, rng, NOISE_PX)
        r = RR.localize(noisy, rec, rig, LC.TAG_INNER)[0]
        assert r["status"] == 0 and r["n_tags"] == 4
        err["rig"].append(pose_err(r["T"]))
        for c, rc in enumerate(rig.cameras):
            s = LR.localize(noisy[c], rec, rc.K, None, LC.TAG_INNER)[0]
            assert s["status"] == 0 and s["n_tags"] == 2
            err[c].append(pose_err(s["T"] @ rc.T_cam_rig))       # world<-camera camera<-rig
    rms = {k: np.sqrt(np.mean(np.square(v), axis=0)) for k, v in err.items()}
    for k in ("rig", 0, 1):
        print("%-4s rotation %.3f mrad, translation %.4f units" % (k, rms[k][0] * 1e3, rms[k][1]))
    for c in (0, 1):
        assert rms["rig"][0] < rms[c][0] and rms["rig"][1] < rms[c][1], (c, rms)


def test_the_covariance_is_consistent_with_the_scatter():
    """as test_pose_cov_ref for one camera: 500 noisy rig solves of the back-to-back frame at 0.3 px, sigma given; the
    mean squared Mahalanobis distance of the world<-rig error under the covariance reported with each solve is 6 +- 5
    standard errors (observed: 6.175, bound 0.77)"""
    tm, rig, poses = RC.back_to_back()
    rec = tm.as_records()
    obs = RC.exact_block(tm, rig, poses[:1], LC.TAG_INNER, 4)
    truth = poses[0]
    rng = np.random.default_rng(505)
    m2 = []
    for _ in range(N_COV):
        out, cov = RR.localize(add_noise(obs, rng, NOISE_PX), rec, rig, LC.TAG_INNER, sigma_px=NOISE_PX)
        assert out["status"][0] == 0 and cov["status"][0] == 0 and cov["dof"][0] == 8 * 4 - 6 and cov["sigma_px"][0] == NOISE_PX
        T = out["T"][0]
        e = PC.pose_error(T[:3, :3], T[:3, 3], truth[:3, :3], truth[:3, 3])
        m2.append(float(e @ np.linalg.solve(cov["cov"][0], e)))
    m2 = np.array(m2)
    print("rig: mean squared Mahalanobis distance %.3f (6 +- %.2f)" % (m2.mean(), COV_BOUND))
    assert abs(m2.mean() - 6.0) <= COV_BOUND, m2.mean()


def test_from_camera_poses_returns_the_mountings():
    c = RC.case("mixed_models")
    rig, truth = c["rig"], c["truth"]
    poses = []
    for rc in rig.cameras:
        p = np.zeros(len(truth), dtype=CAM_POSE_DTYPE)
        p["T"] = [T @ np.linalg.inv(rc.T_cam_rig) for T in truth]       # world<-camera = world<-rig rig<-camera
        poses.append(p)
    poses[1]["status"][2] = 1                   # a frame camera 1 has no pose for is left out
    poses[1]["T"][2] = np.eye(4)
    got = Rig.from_camera_poses([(rc.K, rc.dist) for rc in rig.cameras], poses)
    E0 = rig.cameras[0].T_cam_rig
    assert np.array_equal(got.cameras[0].T_cam_rig, np.eye(4))
    for g, rc in zip(got.cameras, rig.cameras):      # the rig frame is camera 0
        assert np.abs(g.T_cam_rig - rc.T_cam_rig @ np.linalg.inv(E0)).max() <= 1e-9
        assert np.array_equal(g.K, rc.K) and np.array_equal(g.dist, rc.dist)
    poses[1]["status"][:] = 2
    with pytest.raises(ValueError):
        Rig.from_camera_poses([(rc.K, rc.dist) for rc in rig.cameras], poses)


def test_a_mounted_camera_can_be_given_to_the_renderer():
    """rig_cases.synth_camera: the renderer's (position, Euler angles) of a camera given by its 4x4 pose"""
    E1 = RC.mounting(8.0, (6.0, 0.5, 0.0), 1.0)
    for pos, rot in LC.trajectory(16):
        T = LC.world_from_camera(pos, rot) @ np.linalg.inv(E1)
        assert np.abs(LC.world_from_camera(*RC.synth_camera(T)) - T).max() <= 1e-12
        p0, r0 = RC.synth_camera(LC.world_from_camera(pos, rot))
        assert np.allclose(p0, pos, atol=1e-12) and np.allclose(r0, rot, atol=1e-10)


def test_rig_container(tmp_path):
    rig = RC.case("mixed_models")["rig"]
    rec = rig.as_records()
    assert rec.dtype == _lib.RIG_CAMERA_DTYPE and rec.itemsize == 216 and list(rec["n_dist"]) == [0, 5]
    assert np.array_equal(rec["E"][1], rig.cameras[1].T_cam_rig[:3]) and np.array_equal(rec["dist"][1], RC.DIST5) and not rec["dist"][0].any()
    c = np.dtype(rec.dtype.descr, align=True)
    assert c.itemsize == 216 and [c.fields[f][1] for f in c.names] == [rec.dtype.fields[f][1] for f in rec.dtype.names]
    path = str(tmp_path / "rig.npz")
    rig.save(path)
    back = Rig.load(path)
    assert back.as_records().tobytes() == rec.tobytes()
    for a, b in zip(back.cameras, rig.cameras):
        assert a.T_cam_rig.tobytes() == b.T_cam_rig.tobytes() and a.K.tobytes() == b.K.tobytes() and a.dist.tobytes() == b.dist.tobytes()
    assert Rig.from_records(rec).as_records().tobytes() == rec.tobytes()
    bad = np.eye(4)
    bad[0, 0] = 1.001
    for make in (lambda: RigCamera(np.eye(3), np.zeros(3)), lambda: RigCamera(np.eye(3) * np.nan), lambda: RigCamera(np.eye(3), None, bad),
                 lambda: RigCamera(np.eye(3), None, np.diag([1.0, 1.0, -1.0, 1.0])), lambda: Rig([]),
                 lambda: Rig([RigCamera(np.eye(3))] * 17)):
        with pytest.raises(ValueError):
            make()
    for name in ("asl_localize_rig_frames_device", "asl_localize_rig_cov_frames_device", "asl_localize_rig_batch", "asl_localize_rig_cov_batch"):
        assert name in _lib.EXPORTS
