#!/usr/bin/env python3
"""Camera calibration (asl_calibrate_frames_device) on a distorted "webcam" stream: --frames 640x480 frames of a 12-tag 3D
scene through a lens with five coefficients, rendered on the device -> detect -> asl_obs records on the device -> one
calibration.

Prints one JSON line: the solve time (HIP events around the calibration submission alone, median of --reps after
warm-up), per iteration, and the errors against the renderer's camera: fx / fy relative, cx / cy in pixels, the distortion
field's worst pixel difference over a 16 x 16 image grid.

    python tools/calib_lab.py [--frames 1024] [--reps 10] [--iters 30]

--fisheye: the fisheye calibration (asl_calibrate_lens_frames_device, ASL_LENS_FISHEYE) instead, on corners projected on the
host: --frames random views of the 5 x 7 board of tests/calib_fisheye_cases.py through its 640 x 480 lens, float32 corners
with --noise px of Gaussian noise.  The same JSON line, the errors against that lens (the field error over rays within 95
degrees of the axis).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIST = np.array([-0.12, 0.05, 0.002, -0.0015, -0.01])
W, H, FOV, TAG_OUTER, TAG_INNER = 640, 480, 60.0, 18.0, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--max-tags", type=int, default=16)
    ap.add_argument("--fisheye", action="store_true")
    ap.add_argument("--noise", type=float, default=0.3)
    a = ap.parse_args()
    if a.fisheye:
        return fisheye(a)

    import torch

    from aprilslam_amd import _lib, synth
    from aprilslam_amd.calibrate import CALIB_RESULT_DTYPE
    from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap

    dev = torch.device("cuda:0")
    n, mt = a.frames, a.max_tags
    rng = np.random.default_rng(11)
    tags = synth.random_scene(W, H, 12, rng, fov_y_deg=FOV)
    cams = [(tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-4, 4, 3))) for _ in range(n)]
    K = synth.camera_matrix(W, H, FOV)
    rec = TagMap.from_scene(tags).as_records()
    planes, _ = synth.render_planes(W, H, tags, TAG_OUTER, cams, fov_y_deg=FOV, dist=DIST)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_tex = torch.from_numpy(tex).to(dev)
    d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    d_obs = torch.empty((n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty(CALIB_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_poses = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    det.render_frames_device(frames.data_ptr(), n, W, H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2], tex.shape[1],
                             0.5 * TAG_OUTER, K=K, dist=DIST, stream=st)
    det.submit_device(frames.data_ptr(), n, 3, W, H, stream=st)
    det.pack_observations_device(d_obs.data_ptr(), mt, stream=st)
    det.collect()

    def launch():
        det.calibrate_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), TAG_INNER, W, H, d_res.data_ptr(), d_poses.data_ptr(),
                             n_dist=5, max_iters=a.iters, stream=st)

    times = []
    for r in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        stream.synchronize()
        if r >= a.warmup:
            times.append(e0.elapsed_time(e1))
    res = d_res.cpu().numpy().view(CALIB_RESULT_DTYPE)[0]
    import calib_cases as CC
    ms = float(np.median(times))
    print(json.dumps({
        "frames": n, "frames_used": int(res["n_frames_used"]), "corners": int(res["n_corners"]), "status": int(res["status"]),
        "iterations": int(res["iterations"]), "max_iters": a.iters, "ms_per_solve": round(ms, 4),
        "ms_per_iteration": round(ms / a.iters, 5), "rms_px": float(res["rms_px"]), "rms_init_px": float(res["rms_init_px"]),
        "fx_rel_err": float(res["K"][0, 0] / K[0, 0] - 1), "fy_rel_err": float(res["K"][1, 1] / K[1, 1] - 1),
        "cx_err_px": float(res["K"][0, 2] - K[0, 2]), "cy_err_px": float(res["K"][1, 2] - K[1, 2]),
        "dist_field_err_px": CC.field_err(res["K"], res["dist"], K, DIST, W, H), "std": [float(v) for v in res["std"]],
    }))
    det.close()


def fisheye(a):
    import torch

    import calib_fisheye_cases as FC
    from aprilslam_amd import _lib
    from aprilslam_amd.calibrate import CALIB_RESULT_DTYPE
    from aprilslam_amd.localize import CAM_POSE_DTYPE

    dev = torch.device("cuda:0")
    n, mt = a.frames, FC.MAX_TAGS
    rng = np.random.default_rng(11)
    rec = FC.board_map().as_records()
    # (distance, two tilts, roll, turn off axis, its direction), the ranges of the test views
    views = zip(rng.uniform(35, 70, n), rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-180, 180, n), rng.uniform(0, 55, n),
                rng.uniform(0, 360, n))
    obs = np.stack([FC.exact_row(rec, *FC.view_pose(v), FC.K_TRUE, FC.DIST, noise=(rng, a.noise) if a.noise > 0 else None) for v in views])
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_obs = torch.from_numpy(obs.view(np.uint8).copy()).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_res = torch.empty(CALIB_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_poses = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    times = []
    for r in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        det.calibrate_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), FC.LC.TAG_INNER, FC.W, FC.H, d_res.data_ptr(), d_poses.data_ptr(),
                             n_dist=4, max_iters=a.iters, stream=st, model="fisheye")
        e1.record(stream)
        stream.synchronize()
        if r >= a.warmup:
            times.append(e0.elapsed_time(e1))
    res = d_res.cpu().numpy().view(CALIB_RESULT_DTYPE)[0]
    ms = float(np.median(times))
    K = FC.K_TRUE
    print(json.dumps({
        "lens": "fisheye", "frames": n, "frames_used": int(res["n_frames_used"]), "corners": int(res["n_corners"]), "status": int(res["status"]),
        "iterations": int(res["iterations"]), "max_iters": a.iters, "noise_px": a.noise, "ms_per_solve": round(ms, 4),
        "ms_per_iteration": round(ms / a.iters, 5), "rms_px": float(res["rms_px"]), "rms_init_px": float(res["rms_init_px"]),
        "fx_rel_err": float(res["K"][0, 0] / K[0, 0] - 1), "fy_rel_err": float(res["K"][1, 1] / K[1, 1] - 1),
        "cx_err_px": float(res["K"][0, 2] - K[0, 2]), "cy_err_px": float(res["K"][1, 2] - K[1, 2]),
        "dist_field_err_px": FC.field_err(res["K"], res["dist"][:4], K, FC.DIST), "std": [float(v) for v in res["std"]],
    }))
    det.close()


if __name__ == "__main__":
    main()
