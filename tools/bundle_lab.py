#!/usr/bin/env python3
"""Tag bundles (asl_localize_bundles_frames_device, asl_bundle_relative_device): accuracy against a synthetic truth, and one
bundle call against one one-map call per bundle.

B bundles of --tags tags each move independently in front of a moving pinhole camera (1280x720, 45 degrees); a frame's
records hold every tag's exactly projected corners (rounded to float32 as the records hold them), with Gaussian noise of
--noise pixels if asked for, and a PnP pose that is off the truth as a single view's is -- in the manner of
tests/localize_cases.exact_frame.  No image is rendered and no detector runs: the solvers are what is measured.

Accuracy (one JSON line, at --frames frames and --bundles bundles): the error of bundle<-camera and of ref<-bundle (ref 0)
against the truth, rotation in mrad and translation in scene units, RMS over the posed records; and the ratio of the actual
relative-pose error to the reported standard deviation, RMS over the posed pairs and the six components (1 means the
covariance says what the error is; sigma_px is --noise, or estimated from the solves with --noise 0 --estimated).

Timing (one JSON line per F in {1, 1024} x B in {4, 32}): HIP events around (a) the one bundle launch and (b) the B one-map
launches of asl_localize_frames_device back to back, (a) and (b) alternating inside each repetition, median of --reps
after warm-up, plain and with covariance; and whether the two wrote the same bytes.  The events see the host's launch
calls too: B launches from Python cost B ctypes calls, which is part of what the one call saves.

    python tools/bundle_lab.py [--frames 256] [--bundles 8] [--tags 3] [--noise 0.2] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1280, 720
TAG_SIZE = 10.0
FRONTAL = np.diag([1.0, -1.0, -1.0])      # camera<-tag rotation of a tag seen head-on


def rodrigues(r):
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def transform(rvec, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(np.asarray(rvec, dtype=np.float64))
    T[:3, 3] = t
    return T


def pose_error(T_est, T_true):
    """(r, d) with R_true = Rod(r) R_est, p_true = p_est + d: the convention of asl_pose_cov"""
    Q = T_true[:3, :3] @ T_est[:3, :3].T
    w = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]]) / 2
    s = np.linalg.norm(w)
    ang = np.arctan2(s, (np.trace(Q) - 1) / 2)
    return np.concatenate([w * (ang / s) if s > 1e-12 else w, T_true[:3, 3] - T_est[:3, 3]])


def make_bundles(n_bundles, n_tags):
    """a BundleSet of n_bundles layouts of n_tags tags on a ring of radius 9, each a little out of the ring's plane"""
    from aprilslam_amd.bundles import BundleSet
    from aprilslam_amd.localize import TagMap
    maps = []
    for b in range(n_bundles):
        rng = np.random.default_rng(1000 + b)
        poses = {}
        for k in range(n_tags):
            a = 2 * np.pi * k / n_tags
            r = 9.0 if n_tags > 1 else 0.0
            poses[b * n_tags + k] = transform(rng.normal(size=3) * 0.15, (r * np.cos(a), r * np.sin(a), rng.normal() * 1.5))
        maps.append(TagMap(poses))
    return BundleSet(maps)


def make_frames(bundles, n_frames, K, noise, seed=7):
    """(obs (n_frames, max_tags) OBS_DTYPE, truth (n_frames, n_bundles, 4, 4) bundle<-camera): the bundles on a grid in front
    of the camera at a depth that keeps every tag inside the image, each on its own small trajectory, the camera on another"""
    from aprilslam_amd import _lib
    B = len(bundles)
    n_tags = len(bundles.maps[0])
    cols = int(np.ceil(np.sqrt(B * W / H)))
    rows = int(np.ceil(B / cols))
    f_px = K[0, 0]
    cell = 2 * (9.0 + TAG_SIZE) + 8.0                      # a bundle's extent and its motion
    depth = max(f_px * cell * cols / (0.9 * W), f_px * cell * rows / (0.9 * H))
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0, 2 * np.pi, size=(B, 3))
    tilt0 = rng.uniform(-0.4, 0.4, size=(B, 3))
    obs = np.zeros((n_frames, B * n_tags), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    truth = np.zeros((n_frames, B, 4, 4))
    h = float(np.float32(TAG_SIZE / 2))
    obj = np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]])
    for f in range(n_frames):
        t = 2 * np.pi * f / max(n_frames, 16)
        cam = transform((0.02 * np.sin(t), 0.03 * np.cos(t), 0.02 * np.sin(2 * t)), (2.0 * np.cos(t), 1.5 * np.sin(t), 3.0 * np.sin(2 * t)))
        k = 0
        for b, lay in enumerate(bundles.maps):
            cx, cy = (b % cols - (cols - 1) / 2) * cell, (b // cols - (rows - 1) / 2) * cell
            Tcb = np.eye(4)
            Tcb[:3, :3] = rodrigues(tilt0[b] + 0.1 * np.sin(t + phase[b])) @ FRONTAL
            Tcb[:3, 3] = [cx + 3.0 * np.sin(t + phase[b, 0]), cy + 3.0 * np.cos(t + phase[b, 1]), depth + 4.0 * np.sin(t + phase[b, 2])]
            Tcb = cam @ Tcb
            truth[f, b] = np.linalg.inv(Tcb)
            for i in lay.ids():
                T = Tcb @ lay[i]
                P = obj @ T[:3, :3].T + T[:3, 3]
                uv = np.c_[K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]]
                if np.any(P[:, 2] <= 1e-3) or np.any(uv < 0) or np.any(uv[:, 0] >= W) or np.any(uv[:, 1] >= H):
                    continue
                if noise > 0:
                    uv = uv + rng.normal(scale=noise, size=uv.shape)
                T = transform(rng.normal(size=3) * 0.002, rng.normal(size=3) * 0.0005 * np.linalg.norm(T[:3, 3])) @ T
                obs[f, k] = (i, 3, uv.ravel(), T.ravel()[:12])
                k += 1
    return obs, truth


def accuracy(det, bundles, obs, truth, K, sigma_px):
    poses, cov = det.localize_bundles(obs, bundles, K, None, TAG_SIZE, sigma_px=sigma_px)
    rel = det.bundle_relative(poses, cov, 0)
    e_pose = np.array([pose_error(poses["T"][f, b], truth[f, b]) for f, b in zip(*np.nonzero(poses["status"] == 0))])
    ok = np.argwhere((rel["status"] == 0) & (np.arange(rel.shape[1])[None] != 0))
    e_rel, ratio = [], []
    for f, b in ok:
        x = pose_error(rel["T"][f, b], truth[f, 0] @ np.linalg.inv(truth[f, b]))
        e_rel.append(x)
        ratio.append(x / np.sqrt(np.diag(rel["cov"][f, b])))
    e_rel, ratio = np.array(e_rel), np.array(ratio)

    def rms(v):
        return float(np.sqrt(np.mean(np.sum(v * v, axis=1)))) if len(v) else float("nan")
    return {"posed": int((poses["status"] == 0).sum()), "records": int(poses.size), "pairs": int(len(ok)),
            "bundle_from_camera_rot_mrad_rms": 1e3 * rms(e_pose[:, :3]), "bundle_from_camera_trans_rms": rms(e_pose[:, 3:]),
            "ref_from_bundle_rot_mrad_rms": 1e3 * rms(e_rel[:, :3]), "ref_from_bundle_trans_rms": rms(e_rel[:, 3:]),
            "error_over_reported_std_rms": float(np.sqrt(np.mean(ratio * ratio))) if len(ratio) else float("nan"),
            "sigma_px_mean": float(cov["sigma_px"][cov["status"] == 0].mean())}


def timing(det, K, n_frames, n_bundles, n_tags, noise, reps, warmup):
    import torch

    from aprilslam_amd import _lib
    dev = torch.device("cuda:0")
    bundles = make_bundles(n_bundles, n_tags)
    obs, _ = make_frames(bundles, n_frames, K, noise)
    tabs = bundles.table()
    B, n_ids = tabs.shape
    mt = obs.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_obs, d_maps = up(obs), up(tabs)
    pose_b, cov_b, map_b = _lib.CAM_POSE_DTYPE.itemsize, _lib.POSE_COV_DTYPE.itemsize, _lib.MAP_TAG_DTYPE.itemsize
    d_out = torch.zeros((2, n_frames * B * pose_b), dtype=torch.uint8, device=dev)      # [0] the bundle call, [1] B x (n_frames) one-map calls
    d_cov = torch.zeros((2, n_frames * B * cov_b), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream

    def one_call(cov):
        det.localize_bundles_device(d_obs.data_ptr(), n_frames, mt, d_maps.data_ptr(), B, n_ids, d_out[0].data_ptr(), K, None, TAG_SIZE, stream=st,
                                    cov_ptr=d_cov[0].data_ptr() if cov else None)

    def b_calls(cov):
        for b in range(B):
            det.localize_device(d_obs.data_ptr(), n_frames, mt, d_maps.data_ptr() + b * n_ids * map_b, n_ids, d_out[1].data_ptr() + b * n_frames * pose_b,
                                K, None, TAG_SIZE, stream=st, cov_ptr=d_cov[1].data_ptr() + b * n_frames * cov_b if cov else None)

    legs = [("bundle_call", lambda: one_call(0)), ("b_one_map_calls", lambda: b_calls(0)), ("bundle_call_cov", lambda: one_call(1)),
            ("b_one_map_calls_cov", lambda: b_calls(1))]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.cuda.stream(stream):
        for _ in range(warmup):
            for _, fn in legs:
                fn()
        times = {name: [] for name, _ in legs}
        for _ in range(reps):
            for name, fn in legs:        # alternating: every repetition runs each leg once, back to back
                times[name].append(timed(fn))
    stream.synchronize()
    got = d_out[0].cpu().numpy().view(_lib.CAM_POSE_DTYPE).reshape(n_frames, B)
    per = d_out[1].cpu().numpy().view(_lib.CAM_POSE_DTYPE).reshape(B, n_frames)
    gcov = d_cov[0].cpu().numpy().view(_lib.POSE_COV_DTYPE).reshape(n_frames, B)
    pcov = d_cov[1].cpu().numpy().view(_lib.POSE_COV_DTYPE).reshape(B, n_frames)
    line = {"metric": "asl_localize_bundles_frames_device", "frames": n_frames, "bundles": B, "tags_per_bundle": n_tags, "max_tags": mt, "reps": reps,
            "posed": int((got["status"] == 0).sum()),
            "bytes_equal_one_map_calls": bool(np.ascontiguousarray(got.T).tobytes() == per.tobytes() and np.ascontiguousarray(gcov.T).tobytes() == pcov.tobytes())}
    for name, _ in legs:
        line[name + "_ms_median"] = float(np.median(times[name]))
        line[name + "_ms_min"] = float(np.min(times[name]))
    line["speedup_median"] = line["b_one_map_calls_ms_median"] / line["bundle_call_ms_median"]
    line["speedup_cov_median"] = line["b_one_map_calls_cov_ms_median"] / line["bundle_call_cov_ms_median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256, help="frames of the accuracy run")
    ap.add_argument("--bundles", type=int, default=8, help="bundles of the accuracy run")
    ap.add_argument("--tags", type=int, default=3, help="tags per bundle")
    ap.add_argument("--noise", type=float, default=0.2, help="corner noise in pixels (0: exact corners)")
    ap.add_argument("--estimated", action="store_true", help="scale the covariances by the solves' own sigma estimate, not by --noise")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-timing", action="store_true")
    a = ap.parse_args()

    from aprilslam_amd import _lib, synth
    K = synth.camera_matrix(W, H, 45.0)
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    bundles = make_bundles(a.bundles, a.tags)
    obs, truth = make_frames(bundles, a.frames, K, a.noise)
    sigma = 0.0 if (a.estimated or a.noise <= 0) else a.noise
    line = {"metric": "bundle accuracy", "frames": a.frames, "bundles": a.bundles, "tags_per_bundle": a.tags, "noise_px": a.noise, "sigma_px_given": sigma}
    line.update(accuracy(det, bundles, obs, truth, K, sigma))
    print(json.dumps(line), flush=True)
    if not a.no_timing:
        for n_frames in (1, 1024):
            for n_bundles in (4, 32):
                print(json.dumps(timing(det, K, n_frames, n_bundles, a.tags, a.noise, a.reps, a.warmup)), flush=True)
    det.close()


if __name__ == "__main__":
    main()
