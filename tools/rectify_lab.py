"""How long the lens rectification takes: k_rectify's median time for 1024 BGR frames of 1280 x 720, from device events after
a warm-up, next to a device-to-device copy that moves the same number of bytes (the kernel reads 3 B and writes 1 B per
pixel; a copy of 2 B per pixel reads 2 and writes 2).  Prints both and their ratio; nothing is asserted.

    python tools/rectify_lab.py [--frames 1024] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1280, 720
DIST = np.array([-0.12, 0.05, 0.002, -0.0015, -0.01])


def median_ms(fn, reps, warmup, stream):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    from aprilslam_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("rectify_lab needs a GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n = args.frames
    K = synth.camera_matrix(W, H, 45.0)
    src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
    dst = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    copy_src = torch.empty(2 * n * H * W, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    stream = torch.cuda.Stream(dev)
    out = {"frames": n, "width": W, "height": H, "bytes_moved": 4 * n * H * W}
    with torch.cuda.stream(stream):
        for name, ch, nd in (("bgr_lens", 3, 5), ("bgr_no_lens", 3, 0), ("gray_lens", 1, 5)):
            def kernel():
                det.rectify_frames_device(src.data_ptr(), n, ch, W, H, dst.data_ptr(), K, DIST if nd else None, stream=stream.cuda_stream,
                                          stride=3 * W if ch == 3 else W, frame_pitch=3 * W * H)
            out[name + "_ms"] = median_ms(kernel, args.reps, args.warmup, stream)
        out["copy_ms"] = median_ms(lambda: copy_dst.copy_(copy_src, non_blocking=True), args.reps, args.warmup, stream)
    stream.synchronize()
    med, cp = out["bgr_lens_ms"][0], out["copy_ms"][0]
    out["kernel_over_copy"] = med / cp
    out["kernel_GBps"] = out["bytes_moved"] / med * 1e-6
    out["copy_GBps"] = out["bytes_moved"] / cp * 1e-6
    print("k_rectify, %d frames %dx%d BGR, 5 coefficients: median %.3f ms (min %.3f, max %.3f) = %.0f GB/s of its 4 B per pixel" % (
        n, W, H, med, out["bgr_lens_ms"][1], out["bgr_lens_ms"][2], out["kernel_GBps"]))
    print("device-to-device copy of the same bytes: median %.3f ms = %.0f GB/s; kernel / copy = %.2f" % (cp, out["copy_GBps"], med / cp))
    print(json.dumps(out))
    det.close()


if __name__ == "__main__":
    main()
