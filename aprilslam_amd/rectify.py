"""Lens rectification ahead of the detector: the geometry a caller needs around `TagDetector(..., rectify=True)`,
`_lib.Detector.rectify` and `_lib.Detector.rectify_frames_device` (asl_rectify_u8 / asl_rectify_frames_device).

The kernel takes every pixel centre of the rectified image through the inverse of the pinhole K_new, the forward
Brown-Conrady model (k1 k2 p1 p2 k3) and the source camera K, and samples the source there.  Detections on a rectified frame
are therefore in rectified pixels, and their camera is K_new without distortion; `distort_points` takes such points back
into the frame the camera delivered, e.g. to draw on it."""
import numpy as np


def distort_points(pts, K, dist, K_new=None):
    """(..., 2) pixel coordinates in the rectified image (pixel (ix, iy) covers [ix, ix+1) x [iy, iy+1)) -> the same points
    in the source image: the map the rectification kernel samples through.  dist: None or 0, 4 or 5 coefficients
    (k1, k2, p1, p2[, k3]); K_new: the pinhole of the rectified image, default K."""
    p = np.asarray(pts, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    d = np.zeros(0) if dist is None else np.asarray(dist, dtype=np.float64).ravel()
    if len(d) not in (0, 4, 5):
        raise ValueError("dist must hold 0, 4 or 5 coefficients")
    k1, k2, p1, p2, k3 = list(d) + [0.0] * (5 - len(d))
    xn = (p[..., 0] - Kn[0, 2]) / Kn[0, 0]
    yn = (p[..., 1] - Kn[1, 2]) / Kn[1, 1]
    r2 = xn * xn + yn * yn
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=-1)
