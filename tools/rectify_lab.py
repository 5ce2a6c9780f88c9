"""How long the lens rectification takes: k_rectify's median time for 1024 BGR frames of 1280 x 720, from device events after
a warm-up, next to a device-to-device copy that moves the same number of bytes (the kernel reads 3 B and writes 1 B per
pixel; a copy of 2 B per pixel reads 2 and writes 2).  Prints both and their ratio; nothing is asserted.

    python tools/rectify_lab.py [--frames 1024] [--reps 20] [--warmup 3]

--fisheye --views N: what the rotated views of a fisheye cost next to that.  k_rectify_views<3, fisheye> turning every
1280 x 720 BGR frame into N views of 1280 x 720 and k_rectify (the Brown lens, one view of the same size) on the same
frames, alternating in the same run; per-frame times of both, per view for the first, and their ratio.

    python tools/rectify_lab.py --fisheye --views 3 [--frames 256]"""
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


FISH_DIST = np.array([-0.01, 0.003, -0.0005, 0.00002])


def fisheye_main(args):
    import torch

    from aprilslam_amd import _lib, synth
    from aprilslam_amd.rectify import ViewSet
    if not torch.cuda.is_available():
        raise SystemExit("rectify_lab needs a GPU: a time from anywhere else says nothing")
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n, nv = args.frames, args.views
    K_fish = np.array([[0.3 * W, 0.0, 0.5 * W], [0.0, 0.3 * W, 0.5 * H], [0.0, 0.0, 1.0]])   # 1280 px = 191 degrees
    # 90 degree views 60 degrees apart, the fan of the end-to-end test: nearly every output pixel has a sample in the source
    vs = ViewSet.fan(K_fish, FISH_DIST, "fisheye", nv, 90.0, (W, H), step_deg=60.0, theta_max=np.radians(100.0))
    K = synth.camera_matrix(W, H, 45.0)
    src = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev)
    dst = torch.empty((nv, n, H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)

    def fisheye():
        vs.rectify_device(det, src.data_ptr(), n, 3, W, H, dst_ptr=dst.data_ptr(), stream=stream.cuda_stream)

    def brown():
        det.rectify_frames_device(src.data_ptr(), n, 3, W, H, dst.data_ptr(), K, DIST, stream=stream.cuda_stream)

    times = {"fisheye": [], "brown": []}
    with torch.cuda.stream(stream):
        for fn in (fisheye, brown) * args.warmup:
            fn()
        for _ in range(args.reps):      # alternating: whatever else the machine does falls on both alike
            for name, fn in (("fisheye", fisheye), ("brown", brown)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                times[name].append(a.elapsed_time(b))
    fish, brn = float(np.median(times["fisheye"])), float(np.median(times["brown"]))
    filled = float((dst[:, 0] == 0).float().mean().item())
    out = {"frames": n, "views": nv, "width": W, "height": H, "fisheye_ms": fish, "brown_ms": brn, "fisheye_us_per_frame": 1e3 * fish / n,
           "fisheye_us_per_frame_per_view": 1e3 * fish / (n * nv), "brown_us_per_frame": 1e3 * brn / n, "fisheye_over_brown": fish / brn,
           "fisheye_view_over_brown": fish / (nv * brn), "fisheye_min_max_ms": [float(np.min(times["fisheye"])), float(np.max(times["fisheye"]))],
           "brown_min_max_ms": [float(np.min(times["brown"])), float(np.max(times["brown"]))], "share_of_fill_in_frame_0": filled}
    print("k_rectify_views, fisheye, %d views of %dx%d from %d BGR frames: median %.3f ms = %.2f us per frame, %.2f us per frame and view" % (
        nv, W, H, n, fish, out["fisheye_us_per_frame"], out["fisheye_us_per_frame_per_view"]))
    print("k_rectify, Brown, one view: median %.3f ms = %.2f us per frame; fisheye / Brown = %.2f for %d views, %.2f per view" % (
        brn, out["brown_us_per_frame"], out["fisheye_over_brown"], nv, out["fisheye_view_over_brown"]))
    print(json.dumps(out))
    det.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fisheye", action="store_true", help="time the rotated views of a fisheye against the Brown kernel")
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.fisheye:
        return fisheye_main(args)
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
