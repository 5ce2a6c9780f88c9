"""The statement of lens rectification (k_rectify, asl_rectify_frames_device): a distorted BGR or gray frame in, the gray
frame an ideal pinhole K_new would have delivered out.  NumPy, float64, one operation per line; the kernel follows it
operation for operation (no fused multiply-add on either side), so its output is compared byte for byte.

Output pixel (x, y), centre at +0.5 as everywhere in include/aprilslam.h:
  1. normalised coordinates under K_new
  2. forward Brown-Conrady (k1 k2 p1 p2 k3; absent = 0), closed form
  3. source pixel coordinates (u, v) under K
  4. not (0 <= u < w and 0 <= v < h), a NaN included: `fill`
  5. else bilinear, taps clamped to the edge, texel centres at +0.5 (synth._bilinear / render_pixel), floor(o + 0.5)
  6. a BGR tap becomes gray first, with the detector's fixed-point formula (bgr_gray in asl_common.h)
TEST INFRASTRUCTURE: imports nothing from the product."""
import numpy as np


def _coeffs(dist):
    d = np.zeros(0) if dist is None else np.asarray(dist, dtype=np.float64).ravel()
    if len(d) not in (0, 4, 5):
        raise ValueError("dist must hold 0, 4 or 5 coefficients")
    return tuple(float(v) for v in d) + (0.0,) * (5 - len(d))


def _source_coords(px, py, K, dist, K_new):
    """steps 1-3 on pixel coordinates (px, py) of the rectified image (a pixel's centre is its index + 0.5)"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = _coeffs(dist)
    with np.errstate(all="ignore"):
        xn = (px - Kn[0, 2]) / Kn[0, 0]
        yn = (py - Kn[1, 2]) / Kn[1, 1]
        r2 = xn * xn + yn * yn
        rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
        yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
        u = K[0, 0] * xd + K[0, 2]
        v = K[1, 1] * yd + K[1, 2]
    return u, v


def distort_points(pts, K, dist, K_new=None):
    """(..., 2) pixel coordinates in the rectified image -> the same points in the source (distorted) image"""
    p = np.asarray(pts, dtype=np.float64)
    u, v = _source_coords(p[..., 0], p[..., 1], K, dist, K_new)
    return np.stack([u, v], axis=-1)


def bgr_gray(bgr):
    """(..., 3) uint8 BGR -> gray as the detector converts it: (3735 B + 19235 G + 9798 R + 16384) >> 15"""
    a = np.asarray(bgr).astype(np.int64)
    return ((3735 * a[..., 0] + 19235 * a[..., 1] + 9798 * a[..., 2] + 16384) >> 15).astype(np.uint8)


def rectify(src, K, dist, K_new, w_out, h_out, fill=0):
    """src (h, w) or (h, w, 3) uint8 -> (h_out, w_out) uint8 gray"""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3) or (src.ndim == 3 and src.shape[2] != 3):
        raise ValueError("src must be (h, w) or (h, w, 3) uint8")
    gray = (bgr_gray(src) if src.ndim == 3 else src).astype(np.float64)  # converting every tap first = converting the image first
    h, w = gray.shape
    xs, ys = np.meshgrid(np.arange(w_out) + 0.5, np.arange(h_out) + 0.5)
    u, v = _source_coords(xs, ys, K, dist, K_new)
    with np.errstate(invalid="ignore"):
        inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    out = np.full((h_out, w_out), fill, dtype=np.uint8)
    u = u[inside]
    v = v[inside]
    bx = u - 0.5
    by = v - 0.5
    fx0 = np.floor(bx)
    fy0 = np.floor(by)
    fx = bx - fx0
    fy = by - fy0
    ix = fx0.astype(np.int64)
    iy = fy0.astype(np.int64)
    x0c = np.clip(ix, 0, w - 1)
    x1c = np.clip(ix + 1, 0, w - 1)
    y0c = np.clip(iy, 0, h - 1)
    y1c = np.clip(iy + 1, 0, h - 1)
    t00 = gray[y0c, x0c]
    t01 = gray[y0c, x1c]
    t10 = gray[y1c, x0c]
    t11 = gray[y1c, x1c]
    o = t00 * (1 - fx) * (1 - fy) + t01 * fx * (1 - fy) + t10 * (1 - fx) * fy + t11 * fx * fy
    r = np.floor(o + 0.5)
    out[inside] = np.clip(r, 0, 255).astype(np.uint8)
    return out
