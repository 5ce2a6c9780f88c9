#!/usr/bin/env python3
"""Rig mounting calibration (asl_calibrate_rig_frames_device) on a block of exact projections: --cams cameras in a row on one
rig moved along the bench trajectory through the bench scene (rig_cases.exact_block), the mountings of cameras 1 and up
off by 2 degrees and 0.5 units (rig_calib_cases.perturbed).

Prints one JSON line: the time of the whole enqueued solve and, for scale, of one asl_localize_rig_frames_device pass over
the same block (HIP events on one stream around each call, the two alternating inside every repetition, medians of --reps
after --warmup; both calls include the synchronous read-back of the camera table), the trial count, the per-frame
workspace bytes and the mounting errors against the truth.

    python tools/rig_calib_lab.py [--cams 4] [--frames 512] [--max-tags 16] [--reps 10] [--iters 30]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workspace_bytes_per_frame(n_cams):
    """k_rigcal.inc: two poses (12) and two sets of normal equations (28 + 63 ns), the reduced system's share, the
    back-substitution (doubles), the list entry and five ints; ns = n_cams - 1"""
    ns = n_cams - 1
    return 8 * (2 * 12 + 2 * (28 + 63 * ns) + (6 * ns * (6 * ns + 1) // 2 + 6 * ns) + (6 + 36 * ns)) + 4 * 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--max-tags", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()

    import torch

    import localize_cases as LC
    import rig_calib_cases as CC
    import rig_calib_ref as CR
    import rig_cases as RC
    from aprilslam_amd import _lib
    from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap
    from aprilslam_amd.rig import Rig, RigCamera

    dev = torch.device("cuda:0")
    nc, n, mt = a.cams, a.frames, a.max_tags
    tm = TagMap.from_scene(LC.bench_scene())
    rec = tm.as_records()
    truth = Rig([RigCamera(RC.K45, None, RC.mounting(-2.0 * (nc - 1) + 4.0 * c, (-(nc - 1.0) + 2.0 * c, 0.3 * (c % 3), 0.0), 1.0 * (c % 2)))
                 for c in range(nc)])
    poses = [LC.world_from_camera(p, r) for p, r in LC.trajectory(n)]
    obs = RC.exact_block(tm, truth, poses, LC.TAG_INNER, mt)
    rig0 = CC.perturbed(truth, 5).as_records()

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)

    det = _lib.Detector("tagStandard41h12", id_limit=0)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_obs, d_map, d_rig = up(obs), up(rec), up(rig0)
    dts = (_lib.RIG_CAMERA_DTYPE, _lib.RIG_CALIB_RESULT_DTYPE, _lib.POSE_COV_DTYPE, CAM_POSE_DTYPE)
    outs = [torch.zeros(k * dt.itemsize, dtype=torch.uint8, device=dev) for k, dt in zip((nc, 1, nc, n), dts)]
    d_loc = torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def calibrate():
        det.calibrate_rig_device(d_obs.data_ptr(), nc, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), LC.TAG_INNER, outs[0].data_ptr(),
                                 outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), max_iters=a.iters, sigma_px=0.5, stream=st)

    def localize():
        det.localize_rig_device(d_obs.data_ptr(), nc, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_loc.data_ptr(), LC.TAG_INNER, stream=st)

    times = {"calibrate": [], "localize": []}
    for r in range(a.warmup + a.reps):
        for name, fn in (("calibrate", calibrate), ("localize", localize)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = outs[1].cpu().numpy().view(dts[1])[0]
    out = outs[0].cpu().numpy().view(dts[0])
    err = [CR.mounting_error(out["E"][c], truth.cameras[c].T_cam_rig) for c in range(1, nc)]
    err0 = [CR.mounting_error(rig0["E"][c], truth.cameras[c].T_cam_rig) for c in range(1, nc)]
    ms = float(np.median(times["calibrate"]))
    print(json.dumps({
        "cams": nc, "frames": n, "max_tags": mt, "frames_used": int(res["n_frames_used"]), "corners": int(res["n_corners"]),
        "status": int(res["status"]), "n_solved": int(res["n_solved"]), "trials": int(res["iterations"]), "max_iters": a.iters,
        "ms_calibrate": round(ms, 4), "ms_calibrate_min": round(float(np.min(times["calibrate"])), 4),
        "ms_per_trial": round(ms / max(int(res["iterations"]), 1), 5),
        "ms_localize_rig": round(float(np.median(times["localize"])), 4), "ms_localize_rig_min": round(float(np.min(times["localize"])), 4),
        "workspace_bytes_per_frame": workspace_bytes_per_frame(nc),
        "rms_init_px": float(res["rms_init_px"]), "rms_px": float(res["rms_px"]),
        "initial_err_deg_units": [max(e[0] for e in err0), max(e[1] for e in err0)],
        "final_err_deg_units": [max(e[0] for e in err), max(e[1] for e in err)],
    }))
    det.close()


if __name__ == "__main__":
    main()
