#!/usr/bin/env python3
"""Diagnostic: one detector of F families against F one-family detectors on the same frames.

    python tools/multifam_lab.py [--batch 128] [--reps 5] [--decimate 2] [--sets two_widths,four]

Frames: the mixed sheet of tests/multifam_cases.py for the set, tiled up to 1280 x 720 gray, the same frame `batch` times,
resident on the device.  Sets: F = 2 (classic25, circle21) and F = 4 (classic36, classic25, std52, circle21).  The legs are
interleaved (the multi-family detector, then each one-family detector, per repetition); 2 warm-up repetitions, then the
median over `reps` of the isolated per-kernel times (asl_stage_times).  Reported per set: the whole-batch kernel time of
the one detector against the sum over the F detectors, and k_decode_multi against the sum of the F k_decode's (the stage
is called k_decode in both).  Prints one JSON line per set.  Nothing else runs on the GPU meanwhile."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import multifam_cases as MC  # noqa: E402
from aprilslam_amd import _lib  # noqa: E402

W, H = 1280, 720


def tiled(names, decimate):
    sheet = MC.sheet(names, decimate)
    img = np.full((H, W), 255, dtype=np.uint8)
    for y in range(0, H - MC.HEIGHT + 1, MC.HEIGHT):
        for x in range(0, W - MC.WIDTH + 1, MC.WIDTH):
            img[y:y + MC.HEIGHT, x:x + MC.WIDTH] = sheet
    return img


def run(det, d_frames, B, st):
    det.submit_device(d_frames.data_ptr(), B, 1, W, H, stream=st)
    dets, _, npf = det.collect(max_per_frame=512)
    t = {k: v for k, v in det.stage_times().items() if k.startswith("k_")}
    return len(dets), sum(t.values()), t["k_decode"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decimate", type=int, default=2)
    ap.add_argument("--sets", default="two_widths,four", help="keys of multifam_cases.SETS; one_width: three families that share one border width")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    B = args.batch
    for key in args.sets.split(","):
        names = MC.SETS[key]
        fams = list(MC.families(names))
        d_frames = torch.from_numpy(tiled(names, args.decimate)).to(dev)[None].repeat(B, 1, 1).contiguous()
        dets = [_lib.Detector(fams, decimate=float(args.decimate))] + [_lib.Detector(f, decimate=float(args.decimate)) for f in fams]
        for d in dets:
            d.set_profiling(True)
        rows = []
        for it in range(args.reps + 2):
            row = [run(d, d_frames, B, st) for d in dets]  # the legs of one repetition, one after the other
            if it >= 2:
                rows.append(row)
        n = [r[0] for r in rows[0]]
        assert n[0] == sum(n[1:]) > 0, n  # the same tags either way
        med = np.median(np.array([[(r[1], r[2]) for r in row] for row in rows]), axis=0)  # (1 + F, 2)
        print(json.dumps({"set": names, "F": len(names), "batch": B, "decimate": args.decimate, "n_dets": n[0],
                          "all_kernels_ms": {"multi": round(float(med[0, 0]), 4), "singles_sum": round(float(med[1:, 0].sum()), 4),
                                             "singles": [round(float(v), 4) for v in med[1:, 0]]},
                          "decode_ms": {"k_decode_multi": round(float(med[0, 1]), 4), "k_decode_sum": round(float(med[1:, 1].sum()), 4),
                                        "k_decode": [round(float(v), 4) for v in med[1:, 1]]}}))
        for d in dets:
            d.close()


if __name__ == "__main__":
    main()
