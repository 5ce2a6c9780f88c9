"""The statement of rectification into rotated pinhole views (k_rectify_views, asl_rectify_views_device): one frame of a
camera with a lens in, the gray frames of n_views ideal pinholes (K_new, R), each turned against the source camera, out.
NumPy, float64, one operation per line; the kernel follows it operation for operation (no fused multiply-add on either
side), so its output is compared byte for byte.

Output pixel (x, y) of the view (K_new, R), R = source camera <- view, centre at +0.5 as everywhere in include/aprilslam.h:
  1. the view ray dv = ((x + 0.5 - cx') / fx', (y + 0.5 - cy') / fy', 1) and the source ray d = R dv = (X, Y, Z), each
     component r0*dv0 + r1*dv1 + r2*dv2 from left to right
  2. the lens
     LENS_BROWN (n_dist 0, 4 or 5): Z <= 0 gives `fill`; else xn = X / Z, yn = Y / Z and the closed form of
       rectify_ref._source_coords
     LENS_FISHEYE (n_dist 0 or 4: k1 k2 k3 k4, the cv2.fisheye model carried past 90 degrees by the two-argument arctangent):
       r = sqrt(X*X + Y*Y), theta = atan2(r, Z) in [0, pi]; theta > theta_max gives `fill`; t2 = theta*theta,
       theta_d = theta * (1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4)))); s = theta_d / r (r == 0: s = 0);
       u = fx*(s*X) + cx, v = fy*(s*Y) + cy
  3. the outside test, the bilinear tap, the gray conversion and the rounding of rectify_ref.rectify

The arctangent is written out below in + - * /, comparisons and nothing else, because np.arctan2 and a device's atan2 are
each good to an ulp without being the same function: atan2_pos is the function the frames are defined by, on both sides.
TEST INFRASTRUCTURE: imports nothing from the product."""
import numpy as np

import rectify_ref as RR

LENS_BROWN, LENS_FISHEYE = 0, 1
MAX_VIEWS = 16
NEWTON_STEPS = 20

# atan(x) - x = -x^3 (A0 + A1 x^2 + ... + A10 x^20) on |x| <= 7/16, the minimax fit of fdlibm's s_atan.c
A0 = 3.33333333333329318027e-01
A1 = -1.99999999998764832476e-01
A2 = 1.42857142725034663711e-01
A3 = -1.11111104054623557880e-01
A4 = 9.09088713343650656196e-02
A5 = -7.69187620504482999495e-02
A6 = 6.66107313738753120669e-02
A7 = -5.83357013379057348645e-02
A8 = 4.97687799461593236017e-02
A9 = -3.65315727442169155270e-02
A10 = 1.62858201153657823623e-02
# atan(0.5), atan(1), atan(1.5), atan(inf) as the double nearest to each and what it leaves
ATAN_05_HI, ATAN_05_LO = 4.63647609000806093515e-01, 2.26987774529616870924e-17
ATAN_10_HI, ATAN_10_LO = 7.85398163397448278999e-01, 3.06161699786838301793e-17
ATAN_15_HI, ATAN_15_LO = 9.82793723247329054082e-01, 1.39033110312309984516e-17
ATAN_INF_HI, ATAN_INF_LO = 1.57079632679489655800e+00, 6.12323399573676603587e-17
PI_HI, PI_LO = 3.14159265358979311600e+00, 1.22464679914735317723e-16


def atan2_pos(r, Z):
    """atan2(r, Z) for r >= 0, any Z (not -0.0): in [0, pi].  The ratio t = r / |Z| is taken to |x| <= 7/16 by
    atan(t) = atan(c) + atan((t - c) / (1 + c t)) with c one of 0, 0.5, 1, 1.5, inf; Z < 0 mirrors the result in pi/2."""
    r = np.asarray(r, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = np.where(Z < 0, -Z, Z)
        q = r / a
        t = np.where(r == 0, 0.0, q)                      # 0 / 0 too; r > 0 over a == 0 is inf: pi / 2
        x0 = t
        x1 = (2.0 * t - 1.0) / (2.0 + t)
        x2 = (t - 1.0) / (t + 1.0)
        x3 = (t - 1.5) / (1.0 + 1.5 * t)
        x4 = -1.0 / t
        c1 = t < 0.4375
        c2 = t < 0.6875
        c3 = t < 1.1875
        c4 = t < 2.4375
        x = np.where(c1, x0, np.where(c2, x1, np.where(c3, x2, np.where(c4, x3, x4))))
        hi = np.where(c1, 0.0, np.where(c2, ATAN_05_HI, np.where(c3, ATAN_10_HI, np.where(c4, ATAN_15_HI, ATAN_INF_HI))))
        lo = np.where(c1, 0.0, np.where(c2, ATAN_05_LO, np.where(c3, ATAN_10_LO, np.where(c4, ATAN_15_LO, ATAN_INF_LO))))
        z = x * x
        w = z * z
        s1 = z * (A0 + w * (A2 + w * (A4 + w * (A6 + w * (A8 + w * A10)))))
        s2 = w * (A1 + w * (A3 + w * (A5 + w * (A7 + w * A9))))
        p = x * (s1 + s2)
        at = hi - ((p - lo) - x)                          # c1: 0 - ((p - 0) - x) = x - p
        th = np.where(Z < 0, PI_HI - (at - PI_LO), at)
    return th


def _coeffs(dist, model):
    if model == LENS_BROWN:
        return RR._coeffs(dist)
    if model != LENS_FISHEYE:
        raise ValueError("model must be LENS_BROWN or LENS_FISHEYE")
    d = np.zeros(0) if dist is None else np.asarray(dist, dtype=np.float64).ravel()
    if len(d) not in (0, 4):
        raise ValueError("a fisheye lens has 0 or 4 coefficients")
    return tuple(float(v) for v in d) + (0.0,) * (4 - len(d))


def _theta_max(theta_max):
    tm = np.pi if theta_max is None or theta_max == 0 else float(theta_max)
    if not 0 < tm <= np.pi:
        raise ValueError("theta_max must lie in (0, pi]")
    return tm


def source_coords(px, py, K, dist, model, K_new, R, theta_max=None):
    """steps 1-2 on pixel coordinates (px, py) of the view (a pixel's centre is its index + 0.5) -> (u, v) in the source,
    NaN where the lens gives `fill`"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    c = _coeffs(dist, model)
    tm = _theta_max(theta_max)
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    with np.errstate(all="ignore"):
        dv0 = (px - Kn[0, 2]) / Kn[0, 0]
        dv1 = (py - Kn[1, 2]) / Kn[1, 1]
        X = R[0, 0] * dv0 + R[0, 1] * dv1 + R[0, 2] * 1.0
        Y = R[1, 0] * dv0 + R[1, 1] * dv1 + R[1, 2] * 1.0
        Z = R[2, 0] * dv0 + R[2, 1] * dv1 + R[2, 2] * 1.0
        if model == LENS_BROWN:
            k1, k2, p1, p2, k3 = c
            xn = X / Z
            yn = Y / Z
            r2 = xn * xn + yn * yn
            rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
            xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
            yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
            u = K[0, 0] * xd + K[0, 2]
            v = K[1, 1] * yd + K[1, 2]
            gone = Z <= 0
        else:
            k1, k2, k3, k4 = c
            rr = X * X + Y * Y
            r = np.sqrt(rr)
            th = atan2_pos(r, Z)
            t2 = th * th
            td = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r == 0, 0.0, td / r)
            u = K[0, 0] * (s * X) + K[0, 2]
            v = K[1, 1] * (s * Y) + K[1, 2]
            gone = th > tm
        u = np.where(gone, np.nan, u)
        v = np.where(gone, np.nan, v)
    return u, v


def _sample(gray, u, v, w_out, h_out, fill):
    """step 3: rectify_ref.rectify from its outside test on, line for line"""
    h, w = gray.shape
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


def rectify_views(src, K, dist, model, views, w_out, h_out, fill=0, theta_max=None):
    """src (h, w) or (h, w, 3) uint8, views [(K_new, R)] -> (n_views, h_out, w_out) uint8 gray"""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3) or (src.ndim == 3 and src.shape[2] != 3):
        raise ValueError("src must be (h, w) or (h, w, 3) uint8")
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError("1 to %d views" % MAX_VIEWS)
    gray = (RR.bgr_gray(src) if src.ndim == 3 else src).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(w_out) + 0.5, np.arange(h_out) + 0.5)
    out = np.empty((len(views), h_out, w_out), dtype=np.uint8)
    for k, (K_new, R) in enumerate(views):
        u, v = source_coords(xs, ys, K, dist, model, K_new, R, theta_max)
        out[k] = _sample(gray, u, v, w_out, h_out, fill)
    return out


def fisheye_project(rays, K, dist):
    """(..., 3) rays in the source camera's frame -> (..., 2) source pixel coordinates under the fisheye model"""
    d = np.asarray(rays, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    k1, k2, k3, k4 = _coeffs(dist, LENS_FISHEYE)
    X, Y, Z = d[..., 0], d[..., 1], d[..., 2]
    r = np.sqrt(X * X + Y * Y)
    th = atan2_pos(r, Z)
    t2 = th * th
    td = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    with np.errstate(all="ignore"):
        s = np.where(r == 0, 0.0, td / r)
    return np.stack([K[0, 0] * (s * X) + K[0, 2], K[1, 1] * (s * Y) + K[1, 2]], axis=-1)


def fisheye_unproject(u, v, K, dist):
    """source pixel coordinates -> (..., 3) unit rays in the source camera's frame: theta from theta_d by NEWTON_STEPS
    Newton steps from theta = theta_d (no test for convergence: the count is part of the statement)"""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    k1, k2, k3, k4 = _coeffs(dist, LENS_FISHEYE)
    xd = (np.asarray(u, dtype=np.float64) - K[0, 2]) / K[0, 0]
    yd = (np.asarray(v, dtype=np.float64) - K[1, 2]) / K[1, 1]
    td = np.sqrt(xd * xd + yd * yd)
    th = td
    for _ in range(NEWTON_STEPS):
        t2 = th * th
        f = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
        g = 1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4)))
        th = th - f / g
    with np.errstate(all="ignore"):
        q = np.where(td == 0, 0.0, np.sin(th) / td)
    return np.stack([q * xd, q * yd, np.cos(th)], axis=-1)
