#!/usr/bin/env python3
"""Multi-tag camera localisation (asl_localize_frames_device) on the bench workload: 1024 device-rendered 1280x720
frames of the seeded 20-tag scene -> detect + PnP -> asl_obs records on the device -> one camera pose per frame.

Prints one JSON line: the isolated kernel time per 1024 frames (HIP events around the launch alone, median of
--reps after warm-up) and the camera pose error against the renderer's ground truth, single-view (each tag's PnP
composed with the true map) and joint.

    python tools/localize_lab.py [--frames 1024] [--reps 30] [--max-tags 32] [--gate 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-tags", type=int, default=32)
    ap.add_argument("--gate", type=float, default=0.0)
    a = ap.parse_args()

    import torch

    import bench
    from aprilslam_amd import _lib, synth
    from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap

    dev = torch.device("cuda:0")
    W, H, n, mt = bench.W, bench.H, a.frames, a.max_tags
    K = synth.camera_matrix(W, H, 45.0)
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    frames, _, _ = bench.render_stream_device(det, n, dev)
    tags = synth.random_scene(W, H, bench.NTAGS, np.random.default_rng(20250620 + 1), tag_size_outer=bench.TAG_OUTER)
    tm = TagMap.from_scene(tags)
    rec = tm.as_records()
    stream = torch.cuda.Stream(dev)
    d_obs = torch.empty((n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_out = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    det.submit_device(frames.data_ptr(), n, 3, W, H, stream=stream.cuda_stream, K=K, dist=np.zeros(4), tag_size=bench.TAG_INNER)
    det.pack_observations_device(d_obs.data_ptr(), mt, stream=stream.cuda_stream)
    det.collect()

    def launch():
        det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, None, bench.TAG_INNER,
                            max_tag_rms_px=a.gate, stream=stream.cuda_stream)

    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            launch()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    stream.synchronize()
    out = d_out.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, mt)

    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    truths = [np.linalg.inv(flip @ synth.view_matrix(p, r)) for p, r in bench.camera_trajectory(n)]
    jr, jt, sr, st = [], [], [], []
    for f in range(n):
        if out["status"][f] == 0:
            jr.append(rot_err(out["T"][f], truths[f]))
            jt.append(np.linalg.norm(out["T"][f][:3, 3] - truths[f][:3, 3]))
        for o in obs[f][(obs[f]["flags"] & 3) == 3]:
            if o["id"] in tm:
                Tct = np.eye(4)
                Tct[:3] = o["T"].reshape(3, 4)
                Twc = tm[o["id"]] @ np.linalg.inv(Tct)
                sr.append(rot_err(Twc, truths[f]))
                st.append(np.linalg.norm(Twc[:3, 3] - truths[f][:3, 3]))
    rms = lambda v: float(np.sqrt(np.mean(np.square(v)))) if len(v) else None  # noqa: E731
    line = {
        "metric": "asl_localize_frames_device", "frames": n, "max_tags": mt, "tags_per_frame": bench.NTAGS, "gate_px": a.gate,
        "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": float(np.min(ms)), "reps": a.reps,
        "frames_ok": int((out["status"] == 0).sum()), "mean_tags_used": float(out["n_tags"].mean()),
        "mean_rms_px": float(out["rms_px"][out["status"] == 0].mean()),
        "joint": {"rotation_mrad": rms(jr) * 1e3, "translation_mm": rms(jt) * bench.MM_PER_UNIT,
                  "rotation_max_mrad": float(np.max(jr)) * 1e3},
        "single_view": {"rotation_mrad": rms(sr) * 1e3, "translation_mm": rms(st) * bench.MM_PER_UNIT, "poses": len(sr)},
        "note": "camera world<-camera vs the renderer's ground truth; single view = each tag's PnP composed with the true map",
    }
    print(json.dumps(line))
    det.close()


if __name__ == "__main__":
    main()
