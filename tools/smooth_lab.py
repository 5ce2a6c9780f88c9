#!/usr/bin/env python3
"""Sequence localisation (asl_smooth_frames_device) on the bench workload: 1024 device-rendered 1280x720 frames of the
seeded 20-tag scene along the bench trajectory -> detect + PnP -> asl_obs records on the device -> the per-frame
localisation (the seed) -> one smoothed pose per frame.

Prints one JSON line: the time of the smoothing and of the per-frame localisation of the same block (HIP events around each
call alone, the two alternating inside every repetition, median of --reps after warm-up) and the position and rotation
error against the renderer's ground truth before (the per-frame poses) and after.  --drop-every N empties every Nth frame
first, so that the smoothing has holes to fill.  --cov adds the covariance leg: asl_smooth_cov_frames_device timed next
to the plain call, the two alternating inside every repetition (smooth_cov_ms_median / _min), and under "cov" the median
reported std of the frames with data and of the filled ones next to the errors above.  --sequences S adds the block cut into
S equal sequences, solved in one batched call (asl_smooth_sequences_device) and in a loop of S single-sequence device calls,
the legs again alternating inside every repetition ("sequences": batched_ms_median / _min, loop_ms_median / _min, with --cov
both with the covariance; same_bytes: the two wrote the same poses, results and covariances).  --loop-only leaves the batched
call out (a build that does not have it).  --huber K adds the robust call (asl_smooth_robust_sequences_device, Huber threshold
K pixels) on the same input, alternating with the plain one: under "robust" its time, trials, ms per trial next to the plain
call's, n_soft and the position RMSE against the truth next to the plain call's; with --sequences also the batched robust
call.  --outliers N corrupts N taking-part slots first (--outlier-seed): half get one corner moved by 8 px, half the corners
of another slot of their frame.  --jitter J gives frame f the time f + J u_f, u_f uniform in (-0.5, 0.5) (J < 1; 0: unit spacing, the
plain call's bytes) and adds the timed call (asl_smooth_timed_sequences_device) on the same input, alternating with the plain
one: under "timed" its time, trials and position RMSE.  --gap LO:HI drops the frames [LO, HI) and adds three legs, again
alternating: the timed call on the kept frames (their times as above), the naive call (the plain one on the kept frames, the
gap taken for one frame step) and the plain call on all frames with the block emptied; under "gap" the time and trials of each,
the position RMSE of each against the truth over the four frames next to the gap and over all kept frames, and the largest
relative difference of a kept frame's T between the timed and the emptied solve (the same minimum without --jitter; with it the
emptied solve, which has no times, is another problem).  --rig C runs the rig solve instead (asl_smooth_rig_sequences_device): C cameras
side by side on one rig (mountings fanned over 6 degrees of yaw and 2 units), the rig moved along the bench trajectory, every
camera's records from exact projections of the bench scene plus --rig-noise px of corner noise (no rendering: the rig solve
starts from asl_obs blocks); under "rig" the kernel time of the rig localisation and of the rig solve, alternating, and the
rig-smoothed against the per-frame rig position error.

    python tools/smooth_lab.py [--frames 1024] [--reps 20] [--max-tags 32] [--sigma-px 0.3] [--sigma-rot 0.01]
                               [--sigma-trans 0.05] [--max-iters 20] [--drop-every 0] [--cov] [--sequences S [--loop-only]]
                               [--huber K] [--outliers N [--outlier-seed 1]] [--jitter J [--jitter-seed 1]] [--gap LO:HI]
    python tools/smooth_lab.py --rig C [--frames 1024] [--max-tags 2] [--rig-noise 0.3] [--huber K] [--cov] [the sigmas, --max-iters, --reps]
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


def rig_leg(a):
    """--rig C: one JSON line of the rig solve on a synthetic block"""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import localize_cases as LC
    import rig_cases as RC
    from aprilslam_amd import _lib
    from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap
    from aprilslam_amd.rig import Rig, RigCamera

    dev = torch.device("cuda:0")
    n, mt, nc = a.frames, a.max_tags, a.rig
    step = 1.0 / max(1, nc - 1)
    rig = Rig([RigCamera(RC.K45, None, RC.mounting(-3.0 + 6.0 * step * c, (-1.0 + 2.0 * step * c, 0.0, 0.0))) for c in range(nc)])
    tm = TagMap.from_scene(LC.bench_scene())
    rec = tm.as_records()
    truths = [LC.world_from_camera(p, r) for p, r in LC.trajectory(n)]
    obs = RC.exact_block(tm, rig, truths, LC.TAG_INNER, mt)
    rng = np.random.default_rng(1)
    obs["corners"] = (obs["corners"].astype(np.float64) + rng.normal(0.0, a.rig_noise, obs["corners"].shape)).astype(np.float32)
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d_obs, d_map, d_rig = up(obs), up(rec), up(rig.as_records())
    d_seed, d_out = (torch.zeros(n * CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(2))
    d_res = torch.zeros(_lib.SMOOTH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cov = torch.zeros(n * POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def localize_rig():
        det.localize_rig_device(d_obs.data_ptr(), nc, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_seed.data_ptr(), LC.TAG_INNER,
                                stream=stream.cuda_stream)

    def smooth_rig():
        det.smooth_rig_device(d_obs.data_ptr(), nc, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_seed.data_ptr(), d_out.data_ptr(),
                              d_res.data_ptr(), LC.TAG_INNER, sigma_px=a.sigma_px, sigma_rot=a.sigma_rot, sigma_trans=a.sigma_trans,
                              max_iters=a.max_iters, stream=stream.cuda_stream, huber_px=a.huber, cov_ptr=d_cov.data_ptr() if a.cov else None)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs = [localize_rig, smooth_rig]
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for fn in legs:
                fn()
        times = [[] for _ in legs]
        for _ in range(a.reps):
            for k, fn in enumerate(legs):
                times[k].append(timed(fn))
    stream.synchronize()
    seed = d_seed.cpu().numpy().view(CAM_POSE_DTYPE)
    out = d_out.cpu().numpy().view(CAM_POSE_DTYPE)
    res = d_res.cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)[0]
    tr = np.array(truths)

    def rmse(poses, keep):
        return float(np.sqrt(np.mean(np.sum((poses["T"][keep][:, :3, 3] - tr[keep][:, :3, 3]) ** 2, axis=1)))) if keep.any() else None

    posed = seed["status"] == 0
    solved = np.isin(out["status"], (0, 6))
    print(json.dumps({
        "metric": "asl_smooth_rig_sequences_device", "cameras": nc, "frames": n, "max_tags": mt, "corner_noise_px": a.rig_noise,
        "sigma_px": a.sigma_px, "sigma_rot": a.sigma_rot, "sigma_trans": a.sigma_trans, "max_iters": a.max_iters, "huber_px": a.huber,
        "with_cov": bool(a.cov), "reps": a.reps, "slots_per_frame_mean": float(out["n_tags"].mean()),
        "smooth_rig_ms_median": float(np.median(times[1])), "smooth_rig_ms_min": float(np.min(times[1])),
        "localize_rig_ms_median": float(np.median(times[0])), "localize_rig_ms_min": float(np.min(times[0])),
        "ms_per_trial": float(np.median(times[1])) / max(1, int(res["iterations"])),
        "result": {k: (float(res[k]) if res[k].dtype.kind == "f" else int(res[k])) for k in res.dtype.names if k != "reserved"},
        "per_frame_position_rmse_units": rmse(seed, posed), "smoothed_position_rmse_units_same_frames": rmse(out, posed & solved),
        "smoothed_position_rmse_units_all_frames": rmse(out, solved), "frames_without_seed": int((~posed).sum()),
        "note": "world<-rig against the poses the block was projected from; per-frame = asl_localize_rig_frames_device (the seed)"}))
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-tags", type=int, default=32)
    ap.add_argument("--sigma-px", type=float, default=0.3)
    ap.add_argument("--sigma-rot", type=float, default=0.01)
    ap.add_argument("--sigma-trans", type=float, default=0.05)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--drop-every", type=int, default=0)
    ap.add_argument("--cov", action="store_true", help="also time the call with the covariance, alternating with the plain one")
    ap.add_argument("--sequences", type=int, default=0, help="also cut the block into S equal sequences: one batched call against a loop of S calls")
    ap.add_argument("--loop-only", action="store_true", help="with --sequences: time the loop of single calls alone")
    ap.add_argument("--huber", type=float, default=0.0, help="also run the robust call with this Huber threshold in pixels")
    ap.add_argument("--outliers", type=int, default=0, help="corrupt N taking-part slots: half one corner moved by 8 px, half another slot's corners")
    ap.add_argument("--outlier-seed", type=int, default=1)
    ap.add_argument("--jitter", type=float, default=None, help="irregular frame times f + J u, u uniform in (-0.5, 0.5): also run the timed call")
    ap.add_argument("--jitter-seed", type=int, default=1)
    ap.add_argument("--gap", default="", help="LO:HI: drop the frames [LO, HI); timed on the kept frames against naive and against the block emptied")
    ap.add_argument("--rig", type=int, default=0, help="C: the rig solve of C cameras on a synthetic block instead (see the module docstring)")
    ap.add_argument("--rig-noise", type=float, default=0.3, help="with --rig: corner noise in pixels")
    a = ap.parse_args()
    if a.rig:
        if not 1 <= a.rig <= 16 or a.rig * a.max_tags > 256:
            ap.error("--rig C needs 1 <= C <= 16 and C * max-tags <= 256")
        return rig_leg(a)
    if a.sequences and (a.sequences < 1 or a.frames % a.sequences):
        ap.error("--sequences must divide --frames")
    if a.jitter is not None and not 0 <= a.jitter < 1:
        ap.error("--jitter must be in [0, 1): the times have to increase")
    gap = tuple(int(v) for v in a.gap.split(":")) if a.gap else None
    if gap and not (len(gap) == 2 and 2 <= gap[0] < gap[1] <= a.frames - 2):
        ap.error("--gap LO:HI needs 2 <= LO < HI <= frames - 2")

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
    rec = TagMap.from_scene(tags).as_records()
    stream = torch.cuda.Stream(dev)
    d_obs = torch.empty((n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_seed = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_out = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_res = torch.empty(_lib.SMOOTH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cov = torch.empty((n, POSE_COV_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    det.submit_device(frames.data_ptr(), n, 3, W, H, stream=stream.cuda_stream, K=K, dist=np.zeros(4), tag_size=bench.TAG_INNER)
    det.pack_observations_device(d_obs.data_ptr(), mt, stream=stream.cuda_stream)
    det.collect()
    if a.drop_every > 0:
        obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, mt).copy()
        obs["flags"][a.drop_every - 1::a.drop_every] = 0
        d_obs.copy_(torch.from_numpy(obs.view(np.uint8).reshape(n, mt, -1)))

    corrupted = np.zeros(n, dtype=bool)
    if a.outliers > 0:
        obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, mt).copy()
        part = (obs["flags"] & 1).astype(bool) & (obs["id"] >= 0) & (obs["id"] < len(rec))
        part[part] = rec["valid"][obs["id"][part]] != 0
        rng = np.random.default_rng(a.outlier_seed)
        slots = np.argwhere(part)
        pick = slots[rng.choice(len(slots), size=min(a.outliers, len(slots)), replace=False)]
        src = obs["corners"].copy()
        for k, (f, sl) in enumerate(pick):
            others = [o for o in np.flatnonzero(part[f]) if o != sl]
            if k % 2 == 0 or not others:   # one corner moved by 8 px, in a direction of the seed's choosing
                ang = rng.uniform(0.0, 2 * np.pi)
                c = obs["corners"][f, sl].reshape(4, 2)
                c[rng.integers(4)] += np.array([8.0 * np.cos(ang), 8.0 * np.sin(ang)], dtype=np.float32)
            else:                          # the corners of another slot of the frame
                obs["corners"][f, sl] = src[f, others[rng.integers(len(others))]]
            corrupted[f] = True
        d_obs.copy_(torch.from_numpy(obs.view(np.uint8).reshape(n, mt, -1)))

    def localize():
        det.localize_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), K, None, bench.TAG_INNER,
                            stream=stream.cuda_stream)

    def smooth(cov_ptr=None):
        det.smooth_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), K, None,
                          bench.TAG_INNER, sigma_px=a.sigma_px, sigma_rot=a.sigma_rot, sigma_trans=a.sigma_trans, max_iters=a.max_iters,
                          stream=stream.cuda_stream, cov_ptr=cov_ptr)

    def smooth_cov():
        smooth(d_cov.data_ptr())

    d_out_r, d_res_r = torch.zeros_like(d_out), torch.zeros_like(d_res)

    def smooth_robust():
        det.smooth_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), d_out_r.data_ptr(), d_res_r.data_ptr(), K, None,
                          bench.TAG_INNER, sigma_px=a.sigma_px, sigma_rot=a.sigma_rot, sigma_trans=a.sigma_trans, max_iters=a.max_iters,
                          stream=stream.cuda_stream, huber_px=a.huber)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    S = a.sequences
    m = n // S if S else 0
    seq_start = np.arange(S + 1, dtype=np.int32) * m
    if S:   # outputs of their own, so that the two can be compared (the third: the batched robust call's)
        d_outs = [torch.zeros_like(d_out) for _ in range(3)]
        d_ress = [torch.zeros(S * _lib.SMOOTH_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(3)]
        d_covs = [torch.zeros_like(d_cov) for _ in range(3)]
        torch.cuda.synchronize()
    kw = dict(sigma_px=a.sigma_px, sigma_rot=a.sigma_rot, sigma_trans=a.sigma_trans, max_iters=a.max_iters, stream=stream.cuda_stream)

    def batched():
        det.smooth_sequences_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), seq_start, d_outs[0].data_ptr(),
                                    d_ress[0].data_ptr(), K, None, bench.TAG_INNER, cov_ptr=d_covs[0].data_ptr() if a.cov else None, **kw)

    def batched_robust():
        det.smooth_sequences_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), seq_start, d_outs[2].data_ptr(),
                                    d_ress[2].data_ptr(), K, None, bench.TAG_INNER, cov_ptr=d_covs[2].data_ptr() if a.cov else None,
                                    huber_px=a.huber, **kw)

    def loop():
        for k in range(S):
            det.smooth_device(d_obs[k * m:].data_ptr(), m, mt, d_map.data_ptr(), len(rec), d_seed[k * m:].data_ptr(),
                              d_outs[1][k * m:].data_ptr(), d_ress[1][64 * k:].data_ptr(), K, None, bench.TAG_INNER,
                              cov_ptr=d_covs[1][k * m:].data_ptr() if a.cov else None, **kw)

    frame_times = np.arange(n, dtype=np.float64)
    if a.jitter:
        frame_times = frame_times + a.jitter * np.random.default_rng(a.jitter_seed).uniform(-0.5, 0.5, n)
    d_times = torch.from_numpy(frame_times).to(dev)
    d_out_t, d_res_t = torch.zeros_like(d_out), torch.zeros_like(d_res)

    def smooth_timed():
        det.smooth_device(d_obs.data_ptr(), n, mt, d_map.data_ptr(), len(rec), d_seed.data_ptr(), d_out_t.data_ptr(), d_res_t.data_ptr(), K, None,
                          bench.TAG_INNER, times_ptr=d_times.data_ptr(), **kw)

    if gap:   # the kept frames end to end, and all frames with the block emptied; each with the seeds of its own localisation
        kept = np.array([f for f in range(n) if not gap[0] <= f < gap[1]])
        obs_all = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(n, mt)
        emptied = obs_all.copy()
        emptied["flags"][gap[0]:gap[1]] = 0
        nk = len(kept)
        g_obs = [torch.from_numpy(np.ascontiguousarray(o).view(np.uint8).reshape(len(o), mt, -1)).to(dev) for o in (obs_all[kept], emptied)]
        g_seed = [torch.zeros((len(o), CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev) for o in g_obs]
        g_out = [torch.zeros((m_, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev) for m_ in (nk, nk, n)]
        g_res = [torch.zeros_like(d_res) for _ in range(3)]
        g_times = torch.from_numpy(np.ascontiguousarray(frame_times[kept])).to(dev)
        torch.cuda.synchronize()
        for o, sd in zip(g_obs, g_seed):
            det.localize_device(o.data_ptr(), len(o), mt, d_map.data_ptr(), len(rec), sd.data_ptr(), K, None, bench.TAG_INNER, stream=stream.cuda_stream)

        def gap_call(which, k, times_ptr=None):
            det.smooth_device(g_obs[which].data_ptr(), len(g_obs[which]), mt, d_map.data_ptr(), len(rec), g_seed[which].data_ptr(), g_out[k].data_ptr(),
                              g_res[k].data_ptr(), K, None, bench.TAG_INNER, times_ptr=times_ptr, **kw)

        def gap_timed():
            gap_call(0, 0, g_times.data_ptr())

        def gap_naive():
            gap_call(0, 1)

        def gap_emptied():
            gap_call(1, 2)

    legs = [localize, smooth] + ([smooth_cov] if a.cov else []) + ([smooth_robust] if a.huber > 0 else [])
    legs += ([smooth_timed] if a.jitter is not None else []) + ([gap_timed, gap_naive, gap_emptied] if gap else [])
    seq_legs = ([] if a.loop_only else [batched]) + [loop] + ([batched_robust] if a.huber > 0 else []) if S else []
    first_seq_leg = len(legs)
    legs += seq_legs
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for fn in legs:
                fn()
        times = [[] for _ in legs]
        for _ in range(a.reps):
            for k, fn in enumerate(legs):    # alternating: every repetition runs each leg once, back to back
                times[k].append(timed(fn))
    stream.synchronize()
    seed = d_seed.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    out = d_out.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    res = d_res.cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)[0]

    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    truths = [np.linalg.inv(flip @ synth.view_matrix(p, r)) for p, r in bench.camera_trajectory(n)]
    rms = lambda v: float(np.sqrt(np.mean(np.square(v)))) if len(v) else None  # noqa: E731

    def errors(poses, keep):
        fr = np.flatnonzero(keep)
        return {"frames": int(len(fr)), "rotation_mrad": rms([rot_err(poses["T"][f], truths[f]) for f in fr]) * 1e3 if len(fr) else None,
                "translation_mm": rms([np.linalg.norm(poses["T"][f][:3, 3] - truths[f][:3, 3]) for f in fr]) * bench.MM_PER_UNIT if len(fr) else None}

    posed = seed["status"] == 0
    line = {
        "metric": "asl_smooth_frames_device", "frames": n, "max_tags": mt, "tags_per_frame": bench.NTAGS,
        "sigma_px": a.sigma_px, "sigma_rot": a.sigma_rot, "sigma_trans": a.sigma_trans, "max_iters": a.max_iters, "drop_every": a.drop_every,
        "smooth_ms_median": float(np.median(times[1])), "smooth_ms_min": float(np.min(times[1])),
        "localize_ms_median": float(np.median(times[0])), "localize_ms_min": float(np.min(times[0])), "reps": a.reps,
        "result": {k: (float(res[k]) if res[k].dtype.kind == "f" else int(res[k])) for k in res.dtype.names if k != "reserved"},
        "before": errors(seed, posed), "after_same_frames": errors(out, posed & np.isin(out["status"], (0, 6))),
        "after_filled_frames": errors(out, ~posed & np.isin(out["status"], (0, 6))),
        "note": "world<-camera vs the renderer's ground truth; before = the per-frame localisation (the seed)",
    }
    if a.cov:
        cov = d_cov.cpu().numpy().view(POSE_COV_DTYPE).reshape(n)
        std = np.sqrt(np.diagonal(cov["cov"], axis1=1, axis2=2))

        def stds(keep):
            fr = keep & (cov["status"] == 0)
            return {"frames": int(fr.sum()), "rotation_mrad_median": float(np.median(np.linalg.norm(std[fr, :3], axis=1))) * 1e3 if fr.any() else None,
                    "translation_mm_median": float(np.median(np.linalg.norm(std[fr, 3:], axis=1))) * bench.MM_PER_UNIT if fr.any() else None}
        line["smooth_cov_ms_median"], line["smooth_cov_ms_min"] = float(np.median(times[2])), float(np.min(times[2]))
        line["cov"] = {"status": sorted(set(cov["status"].tolist())), "dof": int(cov["dof"][0]),
                       "std_same_frames": stds(posed & np.isin(out["status"], (0, 6))), "std_filled_frames": stds(~posed & np.isin(out["status"], (0, 6))),
                       "note": "median over the frames of |std of the three rotation / translation components|: compare with the RMS errors above"}
    def result(r):
        return {k: (float(r[k]) if r[k].dtype.kind == "f" else int(r[k])) for k in r.dtype.names if k != "reserved"}

    def rmse_units(poses, keep):
        fr = np.flatnonzero(keep)
        return rms([np.linalg.norm(poses["T"][f][:3, 3] - truths[f][:3, 3]) for f in fr])

    if a.outliers > 0:
        line["outliers"] = {"slots": int(len(pick)), "frames": int(corrupted.sum()), "seed": a.outlier_seed}
    if a.huber > 0:
        tr = times[[fn.__name__ for fn in legs].index("smooth_robust")]
        out_r = d_out_r.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
        res_r = d_res_r.cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)[0]
        solved = np.isin(out["status"], (0, 6)) & np.isin(out_r["status"], (0, 6))
        line["robust"] = {"huber_px": a.huber, "smooth_robust_ms_median": float(np.median(tr)), "smooth_robust_ms_min": float(np.min(tr)),
                          "result": result(res_r), "soft_frames": int((out_r["n_rejected"] > 0).sum()),
                          "corrupted_frames_soft": int((out_r["n_rejected"][corrupted] > 0).sum()),
                          "ms_per_trial": float(np.median(tr)) / max(1, int(res_r["iterations"])),
                          "plain_ms_per_trial": float(np.median(times[1])) / max(1, int(res["iterations"])),
                          "position_rmse_units": rmse_units(out_r, solved), "plain_position_rmse_units": rmse_units(out, solved),
                          "seed_position_rmse_units": rmse_units(seed, posed),
                          "after_same_frames": errors(out_r, posed & np.isin(out_r["status"], (0, 6)))}
    leg_times = dict(zip([fn.__name__ for fn in legs], times))
    if a.jitter is not None:
        out_t = d_out_t.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
        res_t = d_res_t.cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)[0]
        solved = np.isin(out["status"], (0, 6)) & np.isin(out_t["status"], (0, 6))
        tt = leg_times["smooth_timed"]
        line["timed"] = {"jitter": a.jitter, "smooth_timed_ms_median": float(np.median(tt)), "smooth_timed_ms_min": float(np.min(tt)),
                         "result": result(res_t), "same_bytes_as_plain": bool(torch.equal(d_out_t, d_out) and torch.equal(d_res_t, d_res)),
                         "ms_per_trial": float(np.median(tt)) / max(1, int(res_t["iterations"])),
                         "plain_ms_per_trial": float(np.median(times[1])) / max(1, int(res["iterations"])),
                         "position_rmse_units": rmse_units(out_t, solved), "plain_position_rmse_units": rmse_units(out, solved)}
    if gap:
        near = [gap[0] - 2, gap[0] - 1, gap[1], gap[1] + 1]
        at = {int(f): i for i, f in enumerate(kept)}
        legs_out = {}
        for k, name in enumerate(("timed", "naive", "emptied")):
            po = g_out[k].cpu().numpy().view(CAM_POSE_DTYPE).reshape(-1)
            rs = g_res[k].cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)[0]
            pos = (lambda f: po["T"][f][:3, 3]) if name == "emptied" else (lambda f: po["T"][at[f]][:3, 3])
            tl = leg_times["gap_" + name]
            legs_out[name] = {"frames": int(len(po)), "ms_median": float(np.median(tl)), "ms_min": float(np.min(tl)), "iterations": int(rs["iterations"]),
                              "status": int(rs["status"]), "rmse_near_units": rms([np.linalg.norm(pos(f) - truths[f][:3, 3]) for f in near]),
                              "rmse_kept_units": rms([np.linalg.norm(pos(int(f)) - truths[int(f)][:3, 3]) for f in kept])}
        Tt = g_out[0].cpu().numpy().view(CAM_POSE_DTYPE).reshape(-1)["T"]
        Te = g_out[2].cpu().numpy().view(CAM_POSE_DTYPE).reshape(-1)["T"][kept]
        seed_near = rms([np.linalg.norm(seed["T"][f][:3, 3] - truths[f][:3, 3]) for f in near])
        line["gap"] = dict(legs_out, lo=gap[0], hi=gap[1], jitter=a.jitter or 0.0, seed_rmse_near_units=seed_near,
                           timed_over_emptied_ms=legs_out["timed"]["ms_median"] / legs_out["emptied"]["ms_median"],
                           timed_against_emptied_rel=float(max(np.abs(x - y).max() / max(1.0, np.abs(y).max()) for x, y in zip(Tt, Te))))
    if S:
        t = dict(zip([fn.__name__ for fn in seq_legs], times[first_seq_leg:]))
        line["sequences"] = {"n_seq": S, "frames_each": m, "with_cov": bool(a.cov),
                             "loop_ms_median": float(np.median(t["loop"])), "loop_ms_min": float(np.min(t["loop"]))}
        if not a.loop_only:
            line["sequences"].update({"batched_ms_median": float(np.median(t["batched"])), "batched_ms_min": float(np.min(t["batched"])),
                                      "loop_over_batched": float(np.median(t["loop"]) / np.median(t["batched"])),
                                      "same_bytes": all(torch.equal(x[0], x[1]) for x in (d_outs, d_ress) + ((d_covs,) if a.cov else ()))})
        r = d_ress[1].cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)
        line["sequences"]["iterations"] = [int(r["iterations"].min()), int(r["iterations"].max())]
        line["sequences"]["status"] = sorted(set(r["status"].tolist()))
        if a.huber > 0:
            rr = d_ress[2].cpu().numpy().view(_lib.SMOOTH_RESULT_DTYPE)
            pr = d_outs[2].cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
            pl = d_outs[1].cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
            solved = np.isin(pr["status"], (0, 6)) & np.isin(pl["status"], (0, 6))
            line["sequences"]["robust"] = {"batched_ms_median": float(np.median(t["batched_robust"])), "batched_ms_min": float(np.min(t["batched_robust"])),
                                           "iterations": [int(rr["iterations"].min()), int(rr["iterations"].max())],
                                           "status": sorted(set(rr["status"].tolist())), "n_soft": int(rr["n_soft"].sum()),
                                           "position_rmse_units": rmse_units(pr, solved), "plain_position_rmse_units": rmse_units(pl, solved)}
    print(json.dumps(line))
    det.close()


if __name__ == "__main__":
    main()
