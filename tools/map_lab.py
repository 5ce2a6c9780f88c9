"""Times asl_map_frames_device (HIP events, median after warm-up) on the bench scene (1024 frames x 20 tags, 720p) and on a
200-tag scene, the host path it replaces (map_init.chain_initial_map + reseed_poses on the host, asl_gn_solve) on the same
observations, and the map and camera errors against the truth in the world-tag gauge.

    python tools/map_lab.py [--frames 1024] [--reps 10] [--out results.json]

With --huber K the robust solve (asl_map_robust_frames_device, huber_px = K) is measured against the plain one on the bench
scene alone: --outliers N slots, spread over the frames, are given their neighbour slot's corners (a mis-decoded id); the
plain and the robust leg alternate, rep by rep, and each reports its map errors against the truth, its trials, its median
total ms and ms per trial, and the robust leg its soft slots.

    python tools/map_lab.py --huber 1.0 --outliers 8 [--iters 60]

With --rig C the rig solve (asl_map_rig_frames_device) of a ring of C cameras (smooth_rig_cases.ring) along the bench trajectory
is measured against the single-camera solve of the ring's camera 0 on the same frames, the two legs alternating rep by rep:
views, pairs, trials, median ms and the map errors against the truth.

    python tools/map_lab.py --rig 2 [--frames 256] [--huber 1.0]

With --cov the covariance solve (asl_mapcov_frames_device) is measured against the same solve without it on the bench scene
and on the 200-tag scene, the two legs alternating rep by rep: median ms of each, their difference (the kept columns of
L^-1 and the Gram kernel), the blocks of the matrix and the bytes of the columns and of the matrix.

    python tools/map_lab.py --cov [--frames 1024] [--huber 1.0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import localize_cases as LC  # noqa: E402
import map_cases as MC  # noqa: E402
import map_ref as MR  # noqa: E402
from aprilslam_amd import _lib, map_init, synth  # noqa: E402


def scene_block(n_frames, ntags, noise, rng):
    K = synth.camera_matrix(LC.W, LC.H, 45.0)
    tags = LC.bench_scene(ntags=ntags)
    cams = LC.trajectory(n_frames)
    mt = min(256, ntags)
    obs = np.stack([LC.exact_frame(tags, p, r, K, max_tags=mt) for p, r in cams])
    obs["corners"] += np.where(obs["id"][..., None] >= 0, rng.normal(0, noise, obs["corners"].shape), 0).astype(np.float32)
    return K, tags, cams, obs


def time_device(det, obs, n_ids, K, reps):
    import torch
    dev = torch.device("cuda:0")
    n, mt = obs.shape
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(n, -1)).to(dev)
    d_map = torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty((n, _lib.CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty((64,), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    ms = []
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        det.build_map_device(d_obs.data_ptr(), n, mt, n_ids, K, None, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                             d_res.data_ptr(), stream=s.cuda_stream)
        b.record(s)
        s.synchronize()
        if r >= 2:
            ms.append(a.elapsed_time(b))
    res = d_res.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(())
    tmap = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(n_ids)
    poses = d_poses.cpu().numpy().view(_lib.CAM_POSE_DTYPE).reshape(n)
    return float(np.median(ms)), res, tmap, poses


def with_outliers(obs, n):
    """n slots, evenly spread over the frames, carry the next slot's corners; the slots changed"""
    out, slots = obs.copy(), []
    F, S = obs.shape
    for k in range(n):
        f = (2 * k + 1) * F // (2 * n)
        s = next(s for s in range((3 * k) % (S - 1), S - 1) if obs["id"][f, s] >= 0 and obs["id"][f, s + 1] >= 0)
        out["corners"][f, s] = obs["corners"][f, s + 1]
        slots.append((f, s))
    return out, slots


def robust_lab(det, a):
    """the plain and the robust leg on the bench scene, alternating"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    K, tags, cams, clean = scene_block(a.frames, 20, 0.3, rng)
    obs, bad = with_outliers(clean, a.outliers) if a.outliers else (clean, [])
    n_ids = 1 + max(t["id"] for t in tags)
    n, mt = obs.shape
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(n, -1)).to(dev)
    d_map = torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty((n, _lib.CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty((64,), dtype=torch.uint8, device=dev)
    d_w = torch.empty((n, mt), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(dev)
    legs = {"plain": dict(), "robust": dict(huber_px=a.huber, slot_weight_ptr=d_w.data_ptr())}
    ms = {k: [] for k in legs}
    out = {}
    for r in range(a.reps + 2):
        for leg, kw in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            det.build_map_device(d_obs.data_ptr(), n, mt, n_ids, K, None, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                                 d_res.data_ptr(), max_iters=a.iters, stream=s.cuda_stream, **kw)
            e1.record(s)
            s.synchronize()
            if r >= 2:
                ms[leg].append(e0.elapsed_time(e1))
            if r == a.reps + 1:
                res = d_res.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(())
                tmap = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(n_ids)
                poses = d_poses.cpu().numpy().view(_lib.CAM_POSE_DTYPE).reshape(n)
                et, er, ec = MC.map_errors(tmap, poses, tags, cams, int(res["world_id"]))
                out[leg] = dict(status=int(res["status"]), trials=int(res["iterations"]), max_iters=a.iters, rms_px=float(res["rms_px"]),
                                tag_err=et, tag_rot_err=er, cam_err=ec, max_std=float(d_std.max().item()), n_soft=int(res["n_soft"]))
                if leg == "robust":
                    w = d_w.cpu().numpy()
                    soft = {(int(f), int(sl)) for f, sl in np.argwhere((w > 0) & (w < 1))}
                    out[leg].update(outliers_soft=len(soft & set(bad)), clean_soft=len(soft - set(bad)))
    for leg in legs:
        out[leg]["ms"] = float(np.median(ms[leg]))
        out[leg]["ms_spread"] = [float(min(ms[leg])), float(max(ms[leg]))]
        out[leg]["ms_per_trial"] = out[leg]["ms"] / max(1, out[leg]["trials"])    # the seed's share included
        out[leg]["ms_per_enqueued_trial"] = out[leg]["ms"] / a.iters               # after the stop a trial is an identity system
    r = dict(frames=n, obs=int((obs["id"] >= 0).sum()), huber_px=a.huber, outliers=len(bad), **out)
    print("robust_lab", json.dumps(r), flush=True)
    return r


def rig_lab(det, a):
    """the rig leg and the single-camera leg (the rig's camera 0) on the bench scene, alternating"""
    import torch
    import map_rig_cases as GC
    import rig_cases as RC
    import smooth_rig_cases as SRC
    dev = torch.device("cuda:0")
    rig = SRC.ring(a.rig) if a.rig > 1 else GC.Rig([GC.RigCamera(RC.K45, None, np.eye(4))])
    mt = min(24, 256 // a.rig)
    poses = GC.bench_poses(a.frames, a.frames)
    obs = GC.add_noise(RC.exact_block(GC.scene(), rig, poses, GC.TAG, mt, pnp_seed=None), 0.3, 7)
    nc, n, _ = obs.shape
    n_ids = GC.N_IDS
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
    d_obs, d_one, d_rig = up(obs), up(obs[0]), up(rig.as_records())
    d_map = torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty((n, _lib.CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty((64,), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    cam0 = rig.cameras[0]
    outs = (d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(), d_res.data_ptr())
    legs = {"rig": lambda: det.build_map_rig_device(d_obs.data_ptr(), nc, n, mt, n_ids, d_rig.data_ptr(), GC.TAG, *outs, max_iters=a.iters,
                                                    stream=s.cuda_stream, huber_px=a.huber),
            "camera0": lambda: det.build_map_device(d_one.data_ptr(), n, mt, n_ids, cam0.K, None, GC.TAG, *outs, max_iters=a.iters,
                                                    stream=s.cuda_stream, huber_px=a.huber)}
    ms = {k: [] for k in legs}
    out = {}
    for r in range(a.reps + 2):
        for leg, call in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            s.synchronize()
            if r >= 2:
                ms[leg].append(e0.elapsed_time(e1))
            if r == a.reps + 1:
                res = d_res.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(())
                tmap = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(n_ids)
                pr = d_poses.cpu().numpy().view(_lib.CAM_POSE_DTYPE).reshape(n)
                truth = poses if leg == "rig" else [T @ np.linalg.inv(cam0.T_cam_rig) for T in poses]
                et, er, ec = GC.truth_errors((res, tmap, None, pr), truth)
                out[leg] = dict(status=int(res["status"]), tags=int(res["n_tags"]), views=int(res["n_obs"]), trials=int(res["iterations"]),
                                rms_px=float(res["rms_px"]), tag_err=et, tag_rot_err=er, pose_err=ec, n_soft=int(res["n_soft"]))
    for leg in legs:
        out[leg]["ms"] = float(np.median(ms[leg]))
        out[leg]["ms_spread"] = [float(min(ms[leg])), float(max(ms[leg]))]
    views, pairs = GC.view_counts(obs)
    r = dict(cameras=nc, frames=n, max_tags=mt, views=views, pairs=pairs, huber_px=a.huber, max_iters=a.iters, **out)
    print("rig_lab", json.dumps(r), flush=True)
    return r


def cov_lab(det, a):
    """the solve without and with the joint covariance, alternating, on both scenes"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    out = {}
    for name, ntags, nf in (("bench_20", 20, a.frames), ("scene_200", 200, min(a.frames, 256))):
        K, tags, cams, obs = scene_block(nf, ntags, 0.3, rng)
        n_ids = 1 + max(t["id"] for t in tags)
        n, mt = obs.shape
        cap = len({int(i) for i in obs["id"].ravel() if i >= 0})
        d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(n, -1)).to(dev)
        d_map = torch.empty((n_ids, _lib.MAP_TAG_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
        d_poses = torch.empty((n, _lib.CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_res = torch.empty((64,), dtype=torch.uint8, device=dev)
        d_slot = torch.empty((n_ids,), dtype=torch.int32, device=dev)
        d_cov = torch.zeros((6 * cap, 6 * cap), dtype=torch.float64, device=dev)
        s = torch.cuda.Stream(dev)
        legs = {"plain": dict(), "cov": dict(cov=(d_slot.data_ptr(), d_cov.data_ptr(), cap))}
        ms = {k: [] for k in legs}
        for r in range(a.reps + 2):
            for leg, kw in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                det.build_map_device(d_obs.data_ptr(), n, mt, n_ids, K, None, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                                     d_res.data_ptr(), max_iters=a.iters, stream=s.cuda_stream, huber_px=a.huber, **kw)
                e1.record(s)
                s.synchronize()
                if r >= 2:
                    ms[leg].append(e0.elapsed_time(e1))
        res = d_res.cpu().numpy().view(_lib.MAP_RESULT_DTYPE).reshape(())
        slot, std, C = d_slot.cpu().numpy(), d_std.cpu().numpy(), d_cov.cpu().numpy()
        nb = int((slot >= 0).sum())
        own = np.concatenate([std[i] for i in np.flatnonzero(slot >= 0)]) if nb else np.zeros(0)
        diag = float(np.abs(np.sqrt(np.diag(C)[:6 * nb]) / own - 1).max()) if nb else 0.0
        n_sys = 6 * int(res["n_tags"])
        r = dict(frames=n, tags=int(res["n_tags"]), status=int(res["status"]), trials=int(res["iterations"]), huber_px=a.huber, blocks=nb,
                 plain_ms=float(np.median(ms["plain"])), plain_ms_spread=[float(min(ms["plain"])), float(max(ms["plain"]))],
                 cov_ms=float(np.median(ms["cov"])), cov_ms_spread=[float(min(ms["cov"])), float(max(ms["cov"]))],
                 cov_extra_ms=float(np.median(np.array(ms["cov"]) - np.array(ms["plain"]))),
                 columns_bytes=8 * n_sys * n_sys, matrix_bytes=8 * 36 * nb * nb, diag_vs_std=diag)
        out[name] = r
        print("cov_lab", name, json.dumps(r), flush=True)
    return out


def time_host(det, obs, K, iters):
    t0 = time.perf_counter()
    frames = [[(int(o["id"]), MR.rec4(o["T"]), o["corners"].astype(np.float64).reshape(4, 2)) for o in fr if o["flags"] & 1 and o["id"] >= 0]
              for fr in obs]
    world, tags, cams = map_init.chain_initial_map(frames)
    ids = sorted(tags)
    cam_idx = [f for f in range(len(frames)) if cams[f] is not None]
    oc, ot, oT, oC = [], [], [], []
    for k, f in enumerate(cam_idx):
        for i, T, c in frames[f]:
            oc.append(k); ot.append(ids.index(i)); oT.append(T); oC.append(c)
    cam_T, tag_T = map_init.reseed_poses(np.array([cams[f] for f in cam_idx]), np.array([tags[i] for i in ids]), oc, ot, oT, oC, K,
                                         LC.TAG_INNER, ids.index(world), sweeps=2, max_cand=8)
    t1 = time.perf_counter()
    cam_T, tag_T, stats = det.gn_solve(cam_T, tag_T, np.array(oc, np.int32), np.array(ot, np.int32), np.array(oC), K, LC.TAG_INNER,
                                       fixed_tag=ids.index(world), iters=iters)
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), world, ids, cam_idx, cam_T, tag_T, stats


def rigid_align(A, B):
    """rotation + translation taking points A (n, 3) onto B, least squares"""
    ca, cb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((A - ca).T @ (B - cb))
    D = np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return lambda X: (X - ca) @ R.T + cb


def errors(tmap, poses, tags, cams, world):
    gt_t, gt_c = MC.truth(tags, cams, world)
    ids = [int(i) for i in np.flatnonzero(tmap["valid"])]
    P = np.array([MR.rec4(tmap["T"][i])[:3, 3] for i in ids])
    Q = np.array([gt_t[i][:3, 3] for i in ids])
    al = rigid_align(P, Q)
    used = np.flatnonzero(poses["status"] == 0)
    C = np.array([poses["T"][f][:3, 3] for f in used])
    Cq = np.array([gt_c[f][:3, 3] for f in used])
    return dict(tag_max=float(np.abs(P - Q).max()), tag_max_aligned=float(np.abs(al(P) - Q).max()),
                cam_max=float(np.abs(C - Cq).max()), cam_max_aligned=float(np.abs(al(C) - Cq).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--huber", type=float, default=0.0, help="huber_px of the robust leg; > 0 runs the plain / robust comparison alone")
    ap.add_argument("--outliers", type=int, default=0, help="slots given their neighbour slot's corners")
    ap.add_argument("--rig", type=int, default=0, help="cameras of the rig; > 0 runs the rig / single-camera comparison alone")
    ap.add_argument("--cov", action="store_true", help="runs the comparison of the solve without and with the joint covariance alone")
    a = ap.parse_args()
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    if a.cov:
        r = cov_lab(det, a)
        det.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        return
    if a.rig > 0:
        r = rig_lab(det, a)
        det.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        return
    if a.huber > 0:
        r = robust_lab(det, a)
        det.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
        return
    rng = np.random.default_rng(7)
    out = {}
    for name, ntags, nf in (("bench_20", 20, a.frames), ("scene_200", 200, min(a.frames, 256))):
        K, tags, cams, obs = scene_block(nf, ntags, 0.3, rng)
        n_ids = 1 + max(t["id"] for t in tags)
        ms, res, tmap, poses = time_device(det, obs, n_ids, K, a.reps)
        hs, hg, world, ids, cam_idx, cam_T, tag_T, stats = time_host(det, obs, K, a.iters)
        hmap = np.zeros(n_ids, dtype=_lib.MAP_TAG_DTYPE)
        for j, i in enumerate(ids):
            hmap["T"][i], hmap["valid"][i] = tag_T[j][:3].ravel(), 1
        hp = np.zeros(nf, dtype=_lib.CAM_POSE_DTYPE)
        hp["status"] = 1
        for k, f in enumerate(cam_idx):
            hp["T"][f], hp["status"][f] = cam_T[k], 0
        r = dict(frames=nf, tags=int(res["n_tags"]), obs=int(res["n_obs"]), status=int(res["status"]), iterations=int(res["iterations"]),
                 rms_px=float(res["rms_px"]), device_ms=ms, host_seed_ms=hs, host_gn_ms=hg, host_cost=float(stats[1]), device_cost=float(res["cost"]),
                 device_err=errors(tmap, poses, tags, cams, int(res["world_id"])), host_err=errors(hmap, hp, tags, cams, world))
        out[name] = r
        print(name, json.dumps(r), flush=True)
    det.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
