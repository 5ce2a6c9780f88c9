"""Multi-tag camera localisation: the NumPy statement (tests/localize_ref.py) on exact projections and on the bench scene
through the CPU oracle detector, the map container and the ABI records.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = synth.camera_matrix(LC.W, LC.H, 45.0)


@pytest.fixture(scope="module")
def scene():
    tags = LC.bench_scene()
    return tags, TagMap.from_scene(tags)


def test_exact_corners_recover_the_pose(scene):
    tags, tm = scene
    cam = LR.camera(K, None)
    for pos, rot in LC.trajectory(16)[:8]:
        truth = LC.world_from_camera(pos, rot)
        # float64 corners: the refinement itself lands on the pose to rounding
        obs = LC.exact_frame(tags, pos, rot, K)
        Xw, uv = [], []
        for o in obs[obs["id"] >= 0]:
            T = synth.camera_from_tag(tags[o["id"]]["position"], tags[o["id"]]["rotation"], pos, rot)
            P = np.c_[LR.object_corners(LC.TAG_INNER), np.zeros(4)] @ T[:3, :3].T + T[:3, 3]
            Xw.append(np.c_[LR.object_corners(LC.TAG_INNER), np.zeros(4), np.ones(4)] @ tm[o["id"]][:3].T)
            uv.append(LR.project(cam, P))
        Xw, uv = np.concatenate(Xw), np.concatenate(uv)
        Tcw = np.linalg.inv(truth)
        start = LR.rodrigues(np.array([0.01, -0.02, 0.015])) @ Tcw[:3, :3], Tcw[:3, 3] + np.array([0.3, -0.2, 0.5])
        R, t, cost = LR.lm(LR.corner_lin(cam, Xw, uv), start[0], start[1])
        est = np.eye(4)
        est[:3, :3], est[:3, 3] = R.T, -(R.T @ t)
        assert LC.rel_err(est, truth) <= 1e-9, LC.rel_err(est, truth)
        # the frame-level statement on the records (corners rounded to float32)
        out = LR.localize(obs[None], tm.as_records(), K, None, LC.TAG_INNER)[0]
        assert out["status"] == 0 and out["n_tags"] == int((obs["id"] >= 0).sum()) and out["n_tags"] >= 10
        assert LC.rel_err(out["T"], truth) <= 1e-5 and out["rms_px"] < 1e-3 and out["n_rejected"] == 0   # float32 corners
        assert 0 <= out["seed_slot"] < len(obs)


def test_statuses_without_tags_or_seeds(scene):
    """the single-camera twin of test_rig_ref's: three exact frames, the covariance statuses through sigma_px"""
    tags, tm = scene
    obs = np.stack([LC.exact_frame(tags, pos, rot, K) for pos, rot in LC.trajectory(16)[:3]])
    obs["flags"][0] = 0               # frame 0: no slot taking part -> status 1
    obs["flags"][1] &= 1              # frame 1: nothing with a PnP -> status 2
    traces = []
    out, cov = LR.localize(obs, tm.as_records(), K, None, LC.TAG_INNER, 0.0, sigma_px=0.5, traces=traces)
    assert list(out["status"]) == [1, 2, 0] and list(cov["status"]) == [1, 1, 0]
    for f in (0, 1):
        assert np.array_equal(out["T"][f], np.eye(4)) and out["n_tags"][f] == 0 and out["seed_slot"][f] == -1
        assert cov["dof"][f] == 0 and cov["sigma_px"][f] == 0.5 and not cov["cov"][f].any()
        assert traces[f] == {"top_k": [], "dropped": [], "gate_rms": [], "active": []}
    assert cov["dof"][2] == 8 * out["n_tags"][2] - 6 and cov["sigma_px"][2] == 0.5 and len(traces[2]["active"]) == out["n_tags"][2]
    assert out.tobytes() == LR.localize(obs, tm.as_records(), K, None, LC.TAG_INNER, 0.0).tobytes()


@pytest.fixture(scope="module")
def oracle_frames(scene):
    """the first 8 of 16 bench trajectory poses, rendered on the host, through the CPU oracle detector + PnP"""
    import oracle_lib as O
    from aprilslam_amd.families import get_family
    tags, _ = scene
    fam = get_family()
    rows, truths = [], []
    for pos, rot in LC.trajectory(16)[:8]:
        frame, _ = synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=pos, cam_rotation_deg=rot)
        dets = [d for d in O.detect_bgr(frame, fam) if d["id"] < len(tags)]
        _, _, T, ok = O.solve_pnp(np.stack([d["corners"] for d in dets]), K, np.zeros(4), LC.TAG_INNER)
        obs = np.zeros(24, dtype=_lib.OBS_DTYPE)
        obs["id"] = -1
        for k, d in enumerate(dets):
            obs["id"][k] = d["id"]
            obs["flags"][k] = 1 | (2 if ok[k] else 0)
            obs["corners"][k] = np.asarray(d["corners"], dtype=np.float32).ravel()
            obs["T"][k] = T[k].ravel()[:12]
        rows.append(obs)
        truths.append(LC.world_from_camera(pos, rot))
    return np.stack(rows), truths


def test_bench_frames_joint_beats_single_view(scene, oracle_frames):
    _, tm = scene
    obs, truths = oracle_frames
    out = LR.localize(obs, tm.as_records(), K, None, LC.TAG_INNER)
    assert (out["status"] == 0).all() and (out["n_tags"] >= 15).all()
    rot = [LC.rot_err(o["T"], t) for o, t in zip(out, truths)]
    tr = [np.linalg.norm(o["T"][:3, 3] - t[:3, 3]) * LC.MM_PER_UNIT for o, t in zip(out, truths)]
    single = []
    for f, truth in enumerate(truths):
        for o in obs[f][(obs[f]["flags"] & 2) != 0]:
            Tct = np.eye(4)
            Tct[:3] = o["T"].reshape(3, 4)
            single.append(LC.rot_err(tm[o["id"]] @ np.linalg.inv(Tct), truth))
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))  # noqa: E731
    assert rms(rot) * 1e3 <= 0.5 and rms(tr) <= 0.5, (rms(rot) * 1e3, rms(tr))
    assert rms(single) * 1e3 >= 20.0, rms(single) * 1e3
    assert (out["rms_px"] < 0.5).all() and (out["rms_px"] <= out["rms_seed_px"]).all()


def test_mirrored_seeds_still_localise(scene):
    tags, tm = scene
    for pos, rot in LC.trajectory(16)[:8]:
        plain = LC.exact_frame(tags, pos, rot, K)
        ref = LR.localize(plain[None], tm.as_records(), K, None, LC.TAG_INNER)[0]
        out = LR.localize(LC.mirror_all(plain)[None], tm.as_records(), K, None, LC.TAG_INNER)[0]
        assert out["status"] == 0 and LC.rel_err(out["T"], ref["T"]) <= 1e-6
        assert LC.rel_err(out["T"], LC.world_from_camera(pos, rot)) <= 1e-5
        assert out["seed_slot"] >= LR.MIRRORED      # every candidate in the right minimum is a mirrored one


def test_gate_drops_a_moved_tag(scene):
    tags, tm = scene
    moved = tm.as_records()
    moved["T"][7][3] += 5.0
    seen = 0
    for pos, rot in LC.trajectory(16)[:8]:
        obs = LC.exact_frame(tags, pos, rot, K)
        if 7 not in obs["id"]:
            continue
        seen += 1
        truth = LC.world_from_camera(pos, rot)
        on = LR.localize(obs[None], moved, K, None, LC.TAG_INNER, max_tag_rms_px=2.0)[0]
        off = LR.localize(obs[None], moved, K, None, LC.TAG_INNER, max_tag_rms_px=0.0)[0]
        assert on["n_rejected"] == 1 and on["n_tags"] == off["n_tags"] - 1 and off["n_rejected"] == 0
        assert LC.rot_err(on["T"], truth) <= 1e-3
        assert LC.rot_err(off["T"], truth) > LC.rot_err(on["T"], truth) and off["rms_px"] > on["rms_px"]
    assert seen >= 4


def test_status_slots_and_ids():
    for name, obs, rec, dist, gate in LC.cpu_cases(K):
        if name == "slots":
            break
    out = LR.localize(obs, rec, K, dist, LC.TAG_INNER, gate)
    assert out["status"][0] == 1 and out["status"][1] == 2
    for f in (0, 1):
        assert np.array_equal(out["T"][f], np.eye(4)) and out["n_tags"][f] == 0 and out["seed_slot"][f] == -1
    taking = lambda f: int(((obs["flags"][f] & 1) != 0).sum() - ((obs["id"][f] >= len(rec)) & ((obs["flags"][f] & 1) != 0)).sum())  # noqa: E731
    assert (out["status"][2:] == 0).all()
    assert out["n_tags"][2] == taking(2)
    assert out["n_tags"][3] == taking(3) and (out["seed_slot"][3] % LR.MIRRORED) % 2 == 0   # PnP-failed odd slots never seed
    assert out["n_tags"][4] == taking(4) and out["seed_slot"][4] >= 5
    cams = LC.trajectory(16)
    for f in (2, 3, 4):
        assert LC.rel_err(out["T"][f], LC.world_from_camera(*cams[f])) <= 1e-5


@pytest.mark.parametrize("n_dist", [0, 4, 5])
def test_distortion_coefficients(scene, n_dist):
    tags, tm = scene
    dist = {0: None, 4: np.array([-0.08, 0.03, 0.0008, -0.0006]), 5: np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])}[n_dist]
    for pos, rot in LC.trajectory(16)[:4]:
        obs = LC.exact_frame(tags, pos, rot, K, dist=dist)
        out = LR.localize(obs[None], tm.as_records(), K, dist, LC.TAG_INNER)[0]
        assert out["status"] == 0 and out["rms_px"] < 1e-3
        assert LC.rel_err(out["T"], LC.world_from_camera(pos, rot)) <= 1e-5
    if n_dist:   # the model matters: the same corners under a pinhole are off
        out = LR.localize(obs[None], tm.as_records(), K, None, LC.TAG_INNER)[0]
        assert out["rms_px"] > 0.1


def test_tag_map_container(scene):
    tags, tm = scene
    assert tm.ids() == list(range(20)) and tm.n_ids == 20 and 7 in tm
    assert np.allclose(tm[3], synth.tag_model_matrix(tags[3]["position"], tags[3]["rotation"]))
    m = TagMap.from_dict({2: np.eye(4), 5: np.eye(4)[:3]})
    rec = m.as_records()
    assert len(rec) == 6 and list(rec["valid"]) == [0, 0, 1, 0, 0, 1] and np.array_equal(rec["T"][5], np.eye(4)[:3].ravel())
    with pytest.raises(ValueError):
        TagMap.from_dict({-1: np.eye(4)})
    with pytest.raises(ValueError):
        TagMap.from_dict({0: np.eye(3)})


def test_map_tag_and_cam_pose_dtypes_match_the_header():
    assert _lib.MAP_TAG_DTYPE.itemsize == 104
    assert CAM_POSE_DTYPE.itemsize == 160
    src = open(os.path.join(ROOT, "include", "aprilslam.h")).read()
    assert re.search(r"\} asl_map_tag;\s*/\*[^*]*104 bytes", src) and re.search(r"\} asl_cam_pose;\s*/\* 160 bytes", src)
    for name in ("asl_localize_frames_device", "asl_localize_batch"):
        assert name in _lib.EXPORTS
