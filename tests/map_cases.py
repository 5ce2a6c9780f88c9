"""Inputs of the map-reconstruction tests (tests/test_map_ref.py on the CPU, tests/test_gpu_map.py on the device):
asl_obs blocks built like localize_cases (exact projections of synth's scenes) and the ground truth in the world-tag
gauge."""
import numpy as np

import localize_cases as LC
import map_ref as MR
from aprilslam_amd import map_init, synth
from aprilslam_amd.localize import TagMap

DIST4 = np.array([-0.08, 0.03, 0.0008, -0.0006])
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
N_IDS = 64


def K_bench():
    return synth.camera_matrix(LC.W, LC.H)


def exact_block(n_frames=12, dist=None, max_tags=24, K=None, tags=None, traj=None):
    """(obs (n_frames, max_tags), tags, camera list) of exact projections of bench_scene along bench's trajectory"""
    K = K_bench() if K is None else K
    tags = LC.bench_scene() if tags is None else tags
    cams = (traj or LC.trajectory(2 * n_frames))[:n_frames]
    obs = np.stack([LC.exact_frame(tags, p, r, K, dist=dist, max_tags=max_tags) for p, r in cams])
    return obs, tags, cams


def truth(tags, cams, world_id):
    """({id: world<-tag}, [world<-camera]) with tag world_id at the identity"""
    tm = TagMap.from_scene(tags)
    Gi = MR.inv(tm[world_id])
    return {i: Gi @ tm[i] for i in tm.ids()}, [Gi @ LC.world_from_camera(p, r) for p, r in cams]


def map_errors(tmap, poses, tags, cams, world_id, tag_size=LC.TAG_INNER):
    """largest tag / camera translation error (scene units) and rotation error (rad) in the world-tag gauge"""
    gt_tags, gt_cams = truth(tags, cams, world_id)
    et = er = 0.0
    for i in np.flatnonzero(tmap["valid"]):
        T = MR.rec4(tmap["T"][i])
        et = max(et, float(np.abs(T[:3, 3] - gt_tags[i][:3, 3]).max()))
        er = max(er, LC.rot_err(T, gt_tags[i]))
    ec = 0.0
    for f, c in enumerate(gt_cams):
        if poses["status"][f] == 0:
            ec = max(ec, float(np.abs(poses["T"][f][:3, 3] - c[:3, 3]).max()))
    return et, er, ec


def two_groups(K=None):
    """frames 0..3 see tags 0..3 only, frames 4..7 tags 10..13 only: no path between the groups"""
    K = K_bench() if K is None else K
    tags = LC.bench_scene()
    obs, _, cams = exact_block(8, K=K, tags=tags)
    ids = sorted({int(i) for i in obs["id"].ravel() if i >= 0})
    keep_a, keep_b = set(ids[:len(ids) // 2]), set(ids[len(ids) // 2:])
    out = obs.copy()
    for f in range(8):
        keep = keep_a if f < 4 else keep_b
        for s in range(out.shape[1]):
            if out["id"][f, s] >= 0 and int(out["id"][f, s]) not in keep:
                out["id"][f, s], out["flags"][f, s] = -1, 0
    return out, tags, cams


FLIP_TAG = 15


def flip_case(K=None):
    """A tag the reseed sweeps cannot repair (obs, tags, cams): 6 frames of a short baseline see tag FLIP_TAG, whose
    records all hold the multi-view second minimum of its pose (the mirror of the truth in its largest view, polished
    against every view), and only its smallest view may seed.  Every candidate the sweeps build is in that basin or
    worse; the flip test's mirror, built in the largest view from the current pose, is in the true one."""
    K = K_bench() if K is None else K
    obs, tags, cams = exact_block(6, K=K, traj=LC.trajectory(256)[:6])
    w = int(min(i for i in obs["id"].ravel() if i >= 0))
    gt, gc = truth(tags, cams, w)
    W = [MR.inv(c) for c in gc]
    views = [(MR.LR.corner_area(obs["corners"][f, s]), f, s) for f, s in zip(*np.nonzero(obs["id"] == FLIP_TAG))]
    _, b, _ = max(views, key=lambda v: (v[0], -v[1]))
    table = MR.rig_ref.rig_table(MR.one_camera(K, None))
    G2, _ = MR.tag_lm(table, [0] * len(views), MR.inv(W[b]) @ MR.mirror4(W[b] @ gt[FLIP_TAG]), [W[f] for _, f, _ in views],
                      [obs["corners"][f, s].astype(np.float64).reshape(4, 2) for _, f, s in views], MR.LR.half_size(LC.TAG_INNER))
    out = obs.copy()
    for _, f, s in views:
        out["T"][f, s] = (W[f] @ G2)[:3].ravel()
        out["flags"][f, s] = 1
    _, f1, s1 = min(views, key=lambda v: (v[0], v[1]))
    out["flags"][f1, s1] = 3
    return out, tags, cams


def cpu_cases(K=None):
    """(name, obs, dist, world_id) of the CPU statement tests, for the kernel comparison"""
    K = K_bench() if K is None else K
    plain, _, _ = exact_block(12, K=K)
    cases = [("exact", plain, None, -1)]
    for nd, dist in ((4, DIST4), (5, DIST5)):
        obs, _, _ = exact_block(12, dist=dist, K=K)
        cases.append(("dist%d" % nd, obs, dist, -1))
    mir = plain.copy()
    w = int(min(i for i in plain["id"].ravel() if i >= 0))
    f, s = np.argwhere(plain["id"] == w)[1]
    mir[f:f + 1, s:s + 1] = LC.mirror_all(plain[f:f + 1, s:s + 1])
    cases.append(("mirrored_world", mir, None, -1))
    cases.append(("two_groups", two_groups(K)[0], None, -1))
    cases.append(("flip", flip_case(K)[0], None, -1))
    odd = plain.copy()
    odd["flags"][0, 1:] = 0                                 # frame 0: one slot -> status 1
    odd["flags"][1, ::2] &= 1                               # frame 1: PnP-failed slots (residuals, no seeds)
    cases.append(("slots", odd, None, -1))
    cases.append(("world_id", plain, None, int(sorted({int(i) for i in plain["id"].ravel() if i >= 0})[3])))
    return cases


def host_path(obs, K, tag_size, iters):
    """map_init.chain_initial_map + reseed_poses + oracle/gn_oracle.py on the same observations (pinhole): (world id,
    tag ids, used frames, world<-camera (n, 4, 4), world<-tag (L, 4, 4), [cost0, cost, accepted])"""
    frames = []
    for f in range(obs.shape[0]):
        frames.append([(int(o["id"]), MR.rec4(o["T"]), o["corners"].astype(np.float64).reshape(4, 2))
                       for o in obs[f] if o["flags"] & 1 and o["id"] >= 0])
    world, tags, cams = map_init.chain_initial_map(frames)
    ids = sorted(tags)
    cam_idx = [f for f in range(len(frames)) if cams[f] is not None]
    oc, ot, oT, oC = [], [], [], []
    for k, f in enumerate(cam_idx):
        for i, T, c in frames[f]:
            oc.append(k); ot.append(ids.index(i)); oT.append(T); oC.append(c)
    cam_T = np.array([cams[f] for f in cam_idx])
    tag_T = np.array([tags[i] for i in ids])
    cam_T, tag_T = map_init.reseed_poses(cam_T, tag_T, oc, ot, oT, oC, K, tag_size, ids.index(world), sweeps=2, max_cand=8)
    cam_T, tag_T, stats = MR.gn_oracle.solve(cam_T, tag_T, np.array(oc), np.array(ot), np.array(oC), K, tag_size, ids.index(world), iters=iters)
    return world, ids, cam_idx, cam_T, tag_T, stats


def host_records(n_ids, n_frames, ids, cam_idx, cam_T, tag_T):
    """host_path's poses as MAP_TAG_DTYPE / CAM_POSE_DTYPE records (for map_errors)"""
    from aprilslam_amd import _lib
    tm = np.zeros(n_ids, dtype=_lib.MAP_TAG_DTYPE)
    for j, i in enumerate(ids):
        tm["T"][i], tm["valid"][i] = tag_T[j][:3].ravel(), 1
    po = np.zeros(n_frames, dtype=_lib.CAM_POSE_DTYPE)
    po["status"] = 1
    for k, f in enumerate(cam_idx):
        po["T"][f], po["status"][f] = cam_T[k], 0
    return tm, po


def webcam_cameras(n, seed=11):
    """test_gpu_calibrate.py's distorted-webcam scene: 12 tags, n random cameras"""
    import calib_cases as CC
    rng = np.random.default_rng(seed)
    tags = synth.random_scene(CC.WEBCAM_W, CC.WEBCAM_H, 12, rng, fov_y_deg=CC.WEBCAM_FOV)
    return tags, [(tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-4, 4, 3))) for _ in range(n)]
