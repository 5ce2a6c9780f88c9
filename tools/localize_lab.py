#!/usr/bin/env python3
"""Multi-tag camera localisation (asl_localize_frames_device) on the bench workload: 1024 device-rendered 1280x720
frames of the seeded 20-tag scene -> detect + PnP -> asl_obs records on the device -> one camera pose per frame.

Prints one JSON line: the isolated kernel time per 1024 frames (HIP events around the launch alone, median of
--reps after warm-up) and the camera pose error against the renderer's ground truth, single-view (each tag's PnP
composed with the true map) and joint.

--cov adds the covariance leg: asl_localize_cov_frames_device timed against the plain call, the two launches alternating
inside every repetition; asl_pose_cov_device over the same records (the per-tag covariance of every slot); and the squared
Mahalanobis distance of the joint pose's error against the ground truth under the reported covariance (6 on average for
Gaussian corner noise of the estimated sigma; detected corners are not that, so it is a finding, not a check).

--map-cov (implies --cov) adds asl_localize_mapcov_frames_device as one more alternating leg: the same call with a joint
covariance of the map carried into the pose covariance.  The map is the true one, so the matrix is a stand-in with the
shape a reconstructed map's has: 2 mrad and 0.05 units per tag, 1 mrad and 0.03 units common to all, the lowest id exact.
It prints the kernel time next to the plain and the _cov ones and how much larger the reported std becomes.

    python tools/localize_lab.py [--frames 1024] [--reps 30] [--max-tags 32] [--gate 0] [--cov] [--map-cov]
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
    ap.add_argument("--cov", action="store_true", help="also time the calls with covariance, interleaved with the plain one")
    ap.add_argument("--map-cov", action="store_true", help="also time the call that carries a map covariance into the pose covariance")
    a = ap.parse_args()
    a.cov = a.cov or a.map_cov

    import torch

    import bench
    from aprilslam_amd import _lib, synth
    from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap

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

    d_cov = torch.empty((n, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_tag_cov = torch.empty((n * mt, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev)

    def launch():
        det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, None, bench.TAG_INNER,
                            max_tag_rms_px=a.gate, stream=stream.cuda_stream)

    def launch_cov():
        det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, None, bench.TAG_INNER,
                            max_tag_rms_px=a.gate, stream=stream.cuda_stream, cov_ptr=d_cov.data_ptr(), sigma_px=0.0)

    def launch_tag_cov():
        det.pose_cov_device(d_obs.data_ptr(), n * mt, d_tag_cov.data_ptr(), K, None, bench.TAG_INNER, 0.0, stream=stream.cuda_stream)

    d_mapcov = torch.empty((n, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    map_ids = sorted(tm.ids())[1:]
    nb = len(map_ids)
    sigma_map = np.kron(np.eye(nb), np.diag([2e-3 ** 2] * 3 + [0.05 ** 2] * 3)) + np.kron(np.ones((nb, nb)), np.diag([1e-3 ** 2] * 3 + [0.03 ** 2] * 3))
    slot = np.full(len(rec), -1, dtype=np.int32)
    slot[map_ids] = np.arange(nb)
    d_sigma, d_slot = torch.from_numpy(sigma_map).to(dev), torch.from_numpy(slot).to(dev)

    def launch_mapcov():
        det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_out.data_ptr(), K, None, bench.TAG_INNER,
                            max_tag_rms_px=a.gate, stream=stream.cuda_stream, cov_ptr=d_mapcov.data_ptr(), sigma_px=0.0,
                            map_cov=(d_sigma.data_ptr(), 6 * nb, d_slot.data_ptr()))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs = [launch] + ([launch_cov, launch_tag_cov] if a.cov else []) + ([launch_mapcov] if a.map_cov else [])
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for fn in legs:
                fn()
        times = [[] for _ in legs]
        for _ in range(a.reps):
            for k, fn in enumerate(legs):    # alternating: every repetition runs each leg once, back to back
                times[k].append(timed(fn))
        ms = times[0]
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
    if a.cov:
        cov = d_cov.cpu().numpy().view(POSE_COV_DTYPE).reshape(n)
        tag_cov = d_tag_cov.cpu().numpy().view(POSE_COV_DTYPE).reshape(n, mt)
        m2 = []
        for f in np.flatnonzero((out["status"] == 0) & (cov["status"] == 0)):
            Q = truths[f][:3, :3] @ out["T"][f][:3, :3].T       # Rod(r) = R_true R^T, d = p_true - p
            w = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]]) / 2
            s = np.sqrt(w @ w)
            r = w * (np.arctan2(s, (np.trace(Q) - 1) / 2) / s) if s > 1e-12 else w
            e = np.concatenate([r, truths[f][:3, 3] - out["T"][f][:3, 3]])
            m2.append(float(e @ np.linalg.solve(cov["cov"][f], e)))
        std = np.sqrt(np.diagonal(cov["cov"][cov["status"] == 0], axis1=1, axis2=2))
        tstd = np.sqrt(np.diagonal(tag_cov["cov"][tag_cov["status"] == 0], axis1=1, axis2=2))
        line["cov"] = {
            "kernel_ms_median": float(np.median(times[1])), "kernel_ms_min": float(np.min(times[1])),
            "plain_ms_median_interleaved": float(np.median(times[0])),
            "pose_cov_records": n * mt, "pose_cov_records_posed": int((tag_cov["status"] == 0).sum()),
            "pose_cov_ms_median": float(np.median(times[2])), "pose_cov_ms_min": float(np.min(times[2])),
            "frames_with_cov": int((cov["status"] == 0).sum()), "sigma_px_median": float(np.median(cov["sigma_px"][cov["status"] == 0])),
            "mahalanobis2_mean": float(np.mean(m2)), "mahalanobis2_median": float(np.median(m2)),
            "joint_std": {"rotation_mrad_median": float(np.median(std[:, :3])) * 1e3,
                          "translation_mm_median": float(np.median(std[:, 3:])) * bench.MM_PER_UNIT},
            "single_tag_std": {"rotation_mrad_median": float(np.median(tstd[:, :3])) * 1e3,
                               "translation_mm_median": float(np.median(tstd[:, 3:])) * bench.MM_PER_UNIT},
            "note": "sigma estimated per solve (sigma_px = 0); chi-square(6) has mean 6, median 5.35",
        }
    if a.map_cov:
        mc = d_mapcov.cpu().numpy().view(POSE_COV_DTYPE).reshape(n)
        both = (cov["status"] == 0) & (mc["status"] == 0)
        ratio = np.sqrt(np.diagonal(mc["cov"][both], axis1=1, axis2=2) / np.diagonal(cov["cov"][both], axis1=1, axis2=2))
        line["map_cov"] = {
            "kernel_ms_median": float(np.median(times[3])), "kernel_ms_min": float(np.min(times[3])),
            "cov_ms_median_interleaved": float(np.median(times[1])), "plain_ms_median_interleaved": float(np.median(times[0])),
            "map_blocks": nb, "frames_with_cov": int((mc["status"] == 0).sum()),
            "std_over_pixel_only_std": {"rotation_median": float(np.median(ratio[:, :3])), "translation_median": float(np.median(ratio[:, 3:]))},
            "note": "a stand-in map covariance: 2 mrad / 0.05 units per tag, 1 mrad / 0.03 units common, lowest id exact",
        }
    print(json.dumps(line))
    det.close()


if __name__ == "__main__":
    main()
