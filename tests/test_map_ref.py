"""The NumPy statement of the tag-map reconstruction (tests/map_ref.py) on exact and broken inputs, against the pinhole host
path it replaces (map_init + oracle/gn_oracle.py), and the product surface (records, exports, TagMap.save / load)."""
import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_ref as MR
from aprilslam_amd import _lib
from aprilslam_amd.localize import TagMap

K = MC.K_bench()


@pytest.mark.parametrize("nd", [0, 4, 5])
def test_exact_projections_give_the_true_map(nd):
    dist = {0: None, 4: MC.DIST4, 5: MC.DIST5}[nd]
    obs, tags, cams = MC.exact_block(12, dist=dist, K=K)
    res, tmap, std, poses = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER)[:4]
    assert res["status"] == 0 and res["rms_px"] < 1e-3
    assert (poses["status"] == 0).all() and res["n_obs_dropped"] == 0
    assert res["world_id"] == min(i for i in obs["id"].ravel() if i >= 0)
    et, er, ec = MC.map_errors(tmap, poses, tags, cams, int(res["world_id"]))
    assert et < 1e-3 and er < 1e-5 and ec < 1e-3, (et, er, ec)
    assert np.array_equal(MR.rec4(tmap["T"][res["world_id"]]), np.eye(4))


def test_no_worse_than_the_pinhole_host_path():
    obs, tags, cams = MC.exact_block(10, K=K)
    rng = np.random.default_rng(3)
    noisy = obs.copy()
    noisy["corners"] += np.where(noisy["id"][..., None] >= 0, rng.normal(0, 0.3, noisy["corners"].shape), 0).astype(np.float32)
    res, tmap, _, poses = MR.map_frames(noisy, MC.N_IDS, K, None, LC.TAG_INNER, max_iters=60, with_std=False)[:4]
    world, ids, cam_idx, cam_T, tag_T, stats = MC.host_path(noisy, K, LC.TAG_INNER, 60)
    assert res["world_id"] == world
    assert res["cost"] <= stats[1] * (1 + 1e-9), (res["cost"], stats[1])
    for j, i in enumerate(ids):
        assert LC.rel_err(MR.rec4(tmap["T"][i]), tag_T[j]) < 1e-6, i
    for k, f in enumerate(cam_idx):
        assert LC.rel_err(poses["T"][f], cam_T[k]) < 1e-6, f


def test_a_mirrored_world_tag_view_is_repaired():
    name, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == "mirrored_world"][0]
    _, tags, cams = MC.exact_block(12, K=K)
    res, tmap, _, poses = MR.map_frames(obs, MC.N_IDS, K, dist, LC.TAG_INNER, with_std=False)[:4]
    assert res["status"] == 0 and res["rms_px"] < 1e-3
    et, er, ec = MC.map_errors(tmap, poses, tags, cams, int(res["world_id"]))
    assert et < 1e-3 and ec < 1e-3


def test_a_tag_mirrored_in_every_view_comes_back():
    # the sweeps alone cannot repair this tag (every candidate they build is in the mirrored basin): it comes back only
    # through the flip test, which must be seen to turn it over
    obs, tags, cams = MC.flip_case(K)
    trace = {}
    res, tmap, _, poses = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, with_std=False, trace=trace)[:4]
    gt, _ = MC.truth(tags, cams, int(res["world_id"]))
    assert trace.get("flipped") == [MC.FLIP_TAG]
    assert res["status"] == 0 and res["rms_px"] < 1e-3
    assert LC.rot_err(MR.rec4(tmap["T"][MC.FLIP_TAG]), gt[MC.FLIP_TAG]) < 1e-5
    # without the flip test's replacement the tag stays in the wrong basin
    keep = MR.tag_lm
    try:
        calls = []

        def no_flip(table, vcs, G, Ws, uvs, h):
            calls.append(1)
            T, c = keep(table, vcs, G, Ws, uvs, h)
            return T, (c if len(calls) % 2 == 1 else np.inf)   # the second call of each tag polishes the mirror
        MR.tag_lm = no_flip
        res2, tmap2, _, _ = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, with_std=False)[:4]
    finally:
        MR.tag_lm = keep
    assert LC.rot_err(MR.rec4(tmap2["T"][MC.FLIP_TAG]), gt[MC.FLIP_TAG]) > 0.1 and res2["rms_px"] > 1e-2


def test_disconnected_groups_and_one_slot_frames():
    obs, _, _ = MC.two_groups(K)
    res, tmap, _, poses = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, with_std=False)[:4]
    assert res["status"] == 0
    assert list(poses["status"]) == [0] * 4 + [5] * 4
    far = {int(i) for i in obs["id"][4:].ravel() if i >= 0}
    assert all(tmap["valid"][i] == 0 for i in far)
    assert res["n_obs_dropped"] == sum(1 for i in obs["id"][4:].ravel() if i >= 0)
    _, odd, _, _ = [c for c in MC.cpu_cases(K) if c[0] == "slots"][0]
    res, _, _, poses = MR.map_frames(odd, MC.N_IDS, K, None, LC.TAG_INNER, with_std=False)[:4]
    assert poses["status"][0] == 1 and poses["seed_slot"][0] == -1 and (poses["status"][1:] == 0).all()


def test_world_id_is_the_identity_and_an_unseen_world_is_nothing_to_solve():
    obs, tags, cams = MC.exact_block(8, K=K)
    ids = sorted({int(i) for i in obs["id"].ravel() if i >= 0})
    res, tmap, _, poses = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, world_id=ids[2], with_std=False)[:4]
    assert res["world_id"] == ids[2] and np.array_equal(MR.rec4(tmap["T"][ids[2]]), np.eye(4))
    missing = next(i for i in range(MC.N_IDS) if i not in ids)
    res, tmap, _, poses = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, world_id=missing, with_std=False)[:4]
    assert res["status"] == 1 and not tmap["valid"].any() and (poses["status"] == 5).all()


def _log_left(Ge, Gr):
    """(omega, v) of the left update taking Gr to Ge: Re = exp(omega) Rr, te = exp(omega) tr + v"""
    R = Ge[:3, :3] @ Gr[:3, :3].T
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (0.5 / np.sinc(th / np.pi) if th > 1e-12 else 0.5)
    return np.concatenate([w, Ge[:3, 3] - MR.gn_oracle.exp_rot(w) @ Gr[:3, 3]])


def test_std_matches_the_spread_of_100_noisy_trials():
    # 6 frames, the 8 nearest tags, 0.1 px of corner noise: per tag and per parameter (omega, v of the left update in the
    # world frame, against the truth in the world-tag gauge) the predicted std is within 0.6-1.6x of the spread.  The std
    # is the linearised one; at 0.3 px one tag of this scene (id 2) already has heavy tails -- a few trials end 6-15 sigma
    # away at the very minimum a start from the truth reaches -- so the check runs where the linearisation holds.
    obs, tags, cams = MC.exact_block(6, K=K, max_tags=8)
    res, tmap, std, _ = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, max_iters=20)[:4]
    w = int(res["world_id"])
    valid = [int(i) for i in np.flatnonzero(tmap["valid"]) if i != w]
    assert len(valid) >= 5 and all(np.all(std[i] > 0) for i in valid) and np.all(std[w] == 0)
    gt, _ = MC.truth(tags, cams, w)
    rng = np.random.default_rng(11)
    err, pred = [], []
    for _ in range(100):
        noisy = obs.copy()
        noisy["corners"] += np.where(noisy["id"][..., None] >= 0, rng.normal(0, 0.1, noisy["corners"].shape), 0).astype(np.float32)
        r, tm, s, _ = MR.map_frames(noisy, MC.N_IDS, K, None, LC.TAG_INNER, max_iters=20)[:4]
        assert r["status"] == 0 and r["world_id"] == w
        err.append([_log_left(MR.rec4(tm["T"][i]), gt[i]) for i in valid])
        pred.append([s[i] for i in valid])
    ratio = np.array(err).std(axis=0) / np.array(pred).mean(axis=0)     # (tags, 6)
    assert ratio.min() > 0.6 and ratio.max() < 1.6, ratio


def test_appending_empty_frames_and_permuting_frames():
    obs, _, _ = MC.exact_block(8, K=K)
    a = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, with_std=False)
    empty = np.zeros((3, obs.shape[1]), dtype=_lib.OBS_DTYPE)
    empty["id"] = -1
    b = MR.map_frames(np.concatenate([obs, empty]), MC.N_IDS, K, None, LC.TAG_INNER, with_std=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[3].tobytes() == b[3][:8].tobytes()
    perm = np.array([3, 0, 7, 5, 1, 6, 2, 4])
    c = MR.map_frames(obs[perm], MC.N_IDS, K, None, LC.TAG_INNER, max_iters=60, with_std=False)
    a60 = MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER, max_iters=60, with_std=False)
    for i in np.flatnonzero(a60[1]["valid"]):
        assert LC.rel_err(MR.rec4(c[1]["T"][i]), MR.rec4(a60[1]["T"][i])) < 1e-8, i


def test_product_surface(tmp_path):
    assert _lib.MAP_RESULT_DTYPE.itemsize == 64
    assert "asl_map_frames_device" in _lib.EXPORTS and "asl_map_batch" in _lib.EXPORTS
    tm = TagMap({3: np.eye(4), 7: MR.rec4(np.arange(12.0) * 0.1)})
    tm.save(tmp_path / "m.npz")
    back = TagMap.load(tmp_path / "m.npz")
    assert back.ids() == [3, 7] and all(np.array_equal(back[i], tm[i]) for i in (3, 7))
    from aprilslam_amd.mapping import MapResult
    obs, _, _ = MC.exact_block(4, K=K)
    r = MapResult(*MR.map_frames(obs, MC.N_IDS, K, None, LC.TAG_INNER)[:4])
    assert r.ok and r.world_id == int(r.result["world_id"]) and len(r.tag_map) == int(r.result["n_tags"])
    assert r.camera_poses.shape == (4, 4, 4) and (r.frame_status == 0).all() and set(r.tag_std) == set(r.tag_map.ids())
