#!/usr/bin/env python3
"""Tag location (asl_locate_tags_frames_device) on the bench workload: 1024 device-rendered 1280x720 frames of the seeded
20-tag scene -> detect + PnP -> asl_obs records on the device -> localisation against the even ids of the scene's map ->
location of the odd ids from those frame poses.

Prints one JSON line: the time of the locate call (its four kernels; HIP events around the call alone, median of --reps
after warm-up) beside the localisation of the same block, the two alternating inside every repetition; and the position /
rotation error of the located tags against the scene, beside the error of the single best view's inv(C_f) T_obs (the view
of largest corner area, its PnP pose composed with the frame's pose).

--rig C: the rig form (asl_locate_tags_rig_frames_device beside asl_localize_rig_frames_device).  C cameras on one rig
follow the bench trajectory, camera 0 at the rig frame and the others fanned out to 6 units and 8 degrees to its right
(C = 2: the rig of tests/test_gpu_rig.py and of the device chain of tests/test_gpu_locate_rig.py, whose block is
--rig 2 --frames 32); every camera's stream is rendered and detected on its own and packed into its part of one
camera-major block.  C * max_tags <= 256.

    python tools/locate_lab.py [--frames 1024] [--reps 30] [--max-tags 32] [--gate 0] [--cov] [--rig C]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rot_err(Ta, Tb):
    R = Ta[:3, :3] @ Tb[:3, :3].T
    return float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def area(c8):
    x, y = c8[0::2].astype(np.float64), c8[1::2].astype(np.float64)
    return 0.5 * abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-tags", type=int, default=32)
    ap.add_argument("--gate", type=float, default=0.0, help="max_view_rms_px of the locate call")
    ap.add_argument("--cov", action="store_true", help="the locate call with the covariance of every located tag")
    ap.add_argument("--rig", type=int, default=0, help="C > 0: C cameras on one rig, the rig forms of both calls")
    a = ap.parse_args()

    import torch

    import bench
    from aprilslam_amd import _lib, synth
    from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap
    from aprilslam_amd.rig import Rig, RigCamera

    dev = torch.device("cuda:0")
    W, H, n, mt = bench.W, bench.H, a.frames, a.max_tags
    K = synth.camera_matrix(W, H, 45.0)
    tags = synth.random_scene(W, H, bench.NTAGS, np.random.default_rng(20250620 + 1), tag_size_outer=bench.TAG_OUTER)
    tm = TagMap.from_scene(tags)
    half_map = tm.as_records()
    half_map[1::2] = np.zeros((), dtype=_lib.MAP_TAG_DTYPE)     # half the tags mapped: the even ids
    ni = len(half_map)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    nc = max(a.rig, 1)
    d_obs = torch.empty((nc, n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map0 = torch.from_numpy(half_map.view(np.uint8)).to(dev)
    d_map = d_map0.clone()
    d_poses = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_fit = torch.empty((ni, _lib.TAG_FIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_cov = torch.empty((ni, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    # the mountings camera_c<-rig, and every camera's own stream into its part of the block
    E = [np.eye(4)]
    if a.rig > 1:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import localize_cases as LC
        import rig_cases as RC
        E = [RC.mounting(8.0 * c / (nc - 1), (6.0 * c / (nc - 1), 0.5 * (c % 2), 0.0), 1.0 * (c % 2)) for c in range(nc)]
    rig = Rig([RigCamera(K, None, Ec) for Ec in E])
    d_rig = torch.from_numpy(rig.as_records().view(np.uint8)).to(dev)
    cams0 = bench.camera_trajectory(n)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    d_tex = torch.from_numpy(tex).to(dev)
    dets = []
    for c in range(nc):
        dc = _lib.Detector("tagStandard41h12", id_limit=0)
        cams = cams0 if c == 0 else [RC.synth_camera(LC.world_from_camera(p, r) @ np.linalg.inv(E[c])) for p, r in cams0]
        planes, _ = synth.render_planes(W, H, tags, bench.TAG_OUTER, cams)
        d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
        frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        dc.render_frames_device(frames.data_ptr(), n, W, H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2], tex.shape[1],
                                0.5 * bench.TAG_OUTER, stream=s)
        dc.submit_device(frames.data_ptr(), n, 3, W, H, stream=s, K=K, dist=np.zeros(4), tag_size=bench.TAG_INNER)
        dc.pack_observations_device(d_obs[c].data_ptr(), mt, stream=s)
        dc.collect()
        dets.append(dc)
        del frames, d_planes
    det = dets[0]

    def localize():
        if a.rig:
            det.localize_rig_device(d_obs.data_ptr(), nc, n, mt, d_map0.data_ptr(), ni, d_rig.data_ptr(), d_poses.data_ptr(), bench.TAG_INNER, stream=s)
        else:
            det.localize_device(d_obs.data_ptr(), n, mt, d_map0.data_ptr(), ni, d_poses.data_ptr(), K, None, bench.TAG_INNER, stream=s)

    def locate():
        cov = dict(cov_ptr=d_cov.data_ptr() if a.cov else None, sigma_px=0.0)
        if a.rig:
            det.locate_tags_rig_device(d_obs.data_ptr(), nc, n, mt, d_poses.data_ptr(), d_map.data_ptr(), ni, d_rig.data_ptr(), d_fit.data_ptr(),
                                       bench.TAG_INNER, max_view_rms_px=a.gate, stream=s, **cov)
        else:
            det.locate_tags_device(d_obs.data_ptr(), n, mt, d_poses.data_ptr(), d_map.data_ptr(), ni, d_fit.data_ptr(), K, None, bench.TAG_INNER,
                                   max_view_rms_px=a.gate, stream=s, **cov)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs = [localize, locate]
    times = [[] for _ in legs]
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            localize()
            d_map.copy_(d_map0)
            locate()
        for _ in range(a.reps):
            for k, fn in enumerate(legs):    # alternating: every repetition runs each leg once, back to back
                if fn is locate:
                    d_map.copy_(d_map0)      # the located entries are valid afterwards: every repetition starts from the half map
                    stream.synchronize()
                times[k].append(timed(fn))
    stream.synchronize()
    fit = d_fit.cpu().numpy().view(_lib.TAG_FIT_DTYPE).reshape(ni)
    out = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(ni)
    poses = d_poses.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(nc, n, mt)

    jp, jr, bp, br = [], [], [], []
    for i in np.flatnonzero(fit["status"] == 0):
        G = np.eye(4)
        G[:3] = out["T"][i].reshape(3, 4)
        jp.append(np.linalg.norm(G[:3, 3] - tm[i][:3, 3]))
        jr.append(rot_err(G, tm[i]))
        best, best_area = None, -1.0
        for f in np.flatnonzero(poses["status"] == 0):
            for c in range(nc):
                for o in obs[c, f][((obs[c, f]["flags"] & 3) == 3) & (obs[c, f]["id"] == i)][:1]:
                    ar = area(o["corners"])
                    if ar > best_area:
                        best, best_area = (f, o, c), ar
        if best is not None:
            Tct = np.eye(4)
            Tct[:3] = best[1]["T"].reshape(3, 4)
            Gb = poses["T"][best[0]] @ np.linalg.inv(E[best[2]]) @ Tct
            bp.append(np.linalg.norm(Gb[:3, 3] - tm[i][:3, 3]))
            br.append(rot_err(Gb, tm[i]))
    rms = lambda v: float(np.sqrt(np.mean(np.square(v)))) if len(v) else None  # noqa: E731
    line = {
        "metric": "asl_locate_tags_rig_frames_device" if a.rig else "asl_locate_tags_frames_device", "n_cams": nc, "frames": n, "max_tags": mt, "n_ids": ni, "gate_px": a.gate, "with_cov": bool(a.cov),
        "locate_ms_median": float(np.median(times[1])), "locate_ms_min": float(np.min(times[1])),
        "localize_ms_median_interleaved": float(np.median(times[0])), "localize_ms_min": float(np.min(times[0])), "reps": a.reps,
        "frames_posed": int((poses["status"] == 0).sum()), "tags_located": int((fit["status"] == 0).sum()),
        "mean_views": float(fit["n_views"][fit["status"] == 0].mean()), "views_rejected": int(fit["n_rejected"].sum()),
        "mean_rms_px": float(fit["rms_px"][fit["status"] == 0].mean()),
        "located": {"position_mm": rms(jp) * bench.MM_PER_UNIT, "position_max_mm": float(np.max(jp)) * bench.MM_PER_UNIT,
                    "rotation_mrad": rms(jr) * 1e3, "rotation_max_mrad": float(np.max(jr)) * 1e3},
        "best_single_view": {"position_mm": rms(bp) * bench.MM_PER_UNIT, "position_max_mm": float(np.max(bp)) * bench.MM_PER_UNIT,
                             "rotation_mrad": rms(br) * 1e3, "rotation_max_mrad": float(np.max(br)) * 1e3},
        "note": "world<-tag of the odd ids vs the scene; best single view = the largest view's PnP pose composed with its frame's pose (a rig: through its camera's mounting)",
    }
    if a.cov:
        cov = d_cov.cpu().numpy().view(POSE_COV_DTYPE).reshape(ni)
        std = np.sqrt(np.diagonal(cov["cov"][cov["status"] == 0], axis1=1, axis2=2))
        line["cov"] = {"tags_with_cov": int((cov["status"] == 0).sum()), "sigma_px_median": float(np.median(cov["sigma_px"][cov["status"] == 0])),
                       "rotation_std_mrad_median": float(np.median(std[:, :3])) * 1e3,
                       "position_std_mm_median": float(np.median(std[:, 3:])) * bench.MM_PER_UNIT}
    print(json.dumps(line))
    for dc in dets:
        dc.close()


if __name__ == "__main__":
    main()
