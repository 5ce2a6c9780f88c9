#!/usr/bin/env python3
"""Rig localisation (asl_localize_rig_frames_device) against the single-camera kernel over the same slots.

The bench workload (1024 device-rendered 1280x720 frames of the seeded 20-tag scene -> detect + PnP) is packed once into
n_cams * max_tags slots per frame.  k_localize reads that block as one camera with n_cams * max_tags slots; the rig
kernel reads the same records regrouped camera-major as n_cams cameras of max_tags slots, every camera with the same K
and the identity mounting -- the same corners in the same global-slot order, so the two solve the same problem and the
difference in time is what the rig form costs (the camera table in LDS, one 3x3 product more per corner).

For every --config CxS: HIP events around each launch alone, the four launches (k_localize, k_localize_rig, and both with
covariance) alternating inside each repetition, median and minimum of --reps after warm-up, and whether the rig poses
are the bytes of the single-camera ones.  One JSON line per configuration.  The rig call reads its camera table back
to check it before the launch (a synchronous copy of n_cams x 216 bytes): that wait lies between the events too.

    python tools/rig_lab.py [--frames 1024] [--reps 30] [--config 2x16 --config 4x8 --config 8x32]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", action="append", help="CxS: C cameras of S slots (default 2x16, 4x8, 8x32)")
    a = ap.parse_args()
    configs = [tuple(int(v) for v in c.split("x")) for c in (a.config or ["2x16", "4x8", "8x32"])]

    import torch

    import bench
    from aprilslam_amd import _lib, synth
    from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap
    from aprilslam_amd.rig import Rig, RigCamera

    dev = torch.device("cuda:0")
    W, H, n = bench.W, bench.H, a.frames
    K = synth.camera_matrix(W, H, 45.0)
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    frames, _, _ = bench.render_stream_device(det, n, dev)
    tags = synth.random_scene(W, H, bench.NTAGS, np.random.default_rng(20250620 + 1), tag_size_outer=bench.TAG_OUTER)
    rec = TagMap.from_scene(tags).as_records()
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    stream = torch.cuda.Stream(dev)
    det.submit_device(frames.data_ptr(), n, 3, W, H, stream=stream.cuda_stream, K=K, dist=np.zeros(4), tag_size=bench.TAG_INNER)
    rec_bytes = _lib.OBS_DTYPE.itemsize
    blocks = {}
    for n_cams, mt in configs:     # one submitted batch, packed at every total slot count
        if n_cams * mt not in blocks:
            blocks[n_cams * mt] = torch.empty((n, n_cams * mt, rec_bytes), dtype=torch.uint8, device=dev)
            det.pack_observations_device(blocks[n_cams * mt].data_ptr(), n_cams * mt, stream=stream.cuda_stream)
    stream.synchronize()
    det.collect()

    for n_cams, mt in configs:
        G = n_cams * mt
        d_single = blocks[G]
        d_rigobs = d_single.view(n, n_cams, mt, rec_bytes).permute(1, 0, 2, 3).contiguous()    # camera-major
        rig = Rig([RigCamera(K, None, np.eye(4)) for _ in range(n_cams)]).as_records()
        d_rig = torch.from_numpy(rig.view(np.uint8).reshape(-1)).to(dev)
        d_out = [torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(4)]
        d_cov = [torch.empty((n, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        st = stream.cuda_stream

        def loc(cov):
            det.localize_device(d_single.data_ptr(), n, G, d_map.data_ptr(), len(rec), d_out[2 * cov].data_ptr(), K, None, bench.TAG_INNER, stream=st,
                                cov_ptr=d_cov[0].data_ptr() if cov else None)

        def rigloc(cov):
            det.localize_rig_device(d_rigobs.data_ptr(), n_cams, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_out[2 * cov + 1].data_ptr(),
                                    bench.TAG_INNER, stream=st, cov_ptr=d_cov[1].data_ptr() if cov else None)

        legs = [("k_localize", lambda: loc(0)), ("k_localize_rig", lambda: rigloc(0)), ("k_localize_cov", lambda: loc(1)),
                ("k_localize_rig_cov", lambda: rigloc(1))]

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                for _, fn in legs:
                    fn()
            times = {name: [] for name, _ in legs}
            for _ in range(a.reps):
                for name, fn in legs:    # alternating: every repetition runs each leg once, back to back
                    times[name].append(timed(fn))
        stream.synchronize()
        outs = [o.cpu().numpy() for o in d_out]
        covs = [c.cpu().numpy() for c in d_cov]
        poses = outs[1].view(CAM_POSE_DTYPE).reshape(n)
        line = {"metric": "asl_localize_rig_frames_device", "frames": n, "n_cams": n_cams, "max_tags": mt, "slots": G, "reps": a.reps,
                "frames_ok": int((poses["status"] == 0).sum()), "mean_tags_used": float(poses["n_tags"].mean()),
                "rig_bytes_equal_single": bool(outs[1].tobytes() == outs[0].tobytes()),
                "rig_cov_bytes_equal_single": bool(outs[3].tobytes() == outs[2].tobytes() and covs[1].tobytes() == covs[0].tobytes())}
        for name, _ in legs:
            line[name + "_ms_median"] = float(np.median(times[name]))
            line[name + "_ms_min"] = float(np.min(times[name]))
        line["rig_over_single_median"] = line["k_localize_rig_ms_median"] / line["k_localize_ms_median"]
        line["rig_cov_over_single_cov_median"] = line["k_localize_rig_cov_ms_median"] / line["k_localize_cov_ms_median"]
        print(json.dumps(line), flush=True)
    det.close()


if __name__ == "__main__":
    main()
