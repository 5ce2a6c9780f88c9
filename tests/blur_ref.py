"""NumPy statement of the detector's quad_sigma stage: upstream AprilTag 3's blur / sharpening of the decimated image.

This file is the definition that k_quad_blur (aprilslam_amd/csrc/k_blur.inc) and asl_blur_taps are held to, bit for bit.

Taps.  sigma = |float32(quad_sigma)|; ksz = int(4 * sigma), the product taken in float32 and truncated, plus 1 if even;
ksz <= 1 is "off".  Otherwise dk[i] = exp(-0.5 * ((i - ksz // 2) / sigma) ** 2) in float64, normalised by its sum (added
left to right), and k[i] = uint8(floor(255 * dk[i])).  Nothing is rounded: the taps sum to a little under 256 and the
image darkens slightly.

Filter.  Separable, rows first, then the columns of that result.  Along a line of n pixels, with r = ksz // 2, pixel i is
(sum_j k[j] * line[i - r + j]) >> 8 for r <= i <= n - r - 2 and a copy otherwise: r pixels at the start, r + 1 at the end
(the asymmetry is upstream's); a line of n <= ksz pixels is copied whole.  quad_sigma > 0 gives the filtered image,
quad_sigma < 0 the sharpened one, clip(2 * image - filtered, 0, 255).
"""
import numpy as np


def blur_taps(quad_sigma):
    """uint8[ksz]; empty = off"""
    sigma = np.abs(np.float32(quad_sigma))
    ksz = int(np.float32(4.0) * sigma)
    if ksz % 2 == 0:
        ksz += 1
    if ksz <= 1:
        return np.zeros(0, np.uint8)
    s = float(sigma)
    dk = np.array([np.exp(-0.5 * (float(i - ksz // 2) / s) ** 2) for i in range(ksz)], dtype=np.float64)
    total = 0.0
    for v in dk:
        total += float(v)
    return np.floor(dk / total * 255.0).astype(np.uint8)


def _filter_rows(a, k):
    """every row of the uint8 image a with the taps k"""
    n, ksz = a.shape[1], len(k)
    r = ksz // 2
    out = a.copy()
    m = n - 2 * r - 1  # filtered pixels: r .. n - r - 2
    if m <= 0:
        return out
    acc = np.zeros((a.shape[0], m), np.uint32)
    for j in range(ksz):
        acc += np.uint32(k[j]) * a[:, j:j + m].astype(np.uint32)
    out[:, r:r + m] = (acc >> 8).astype(np.uint8)
    return out


def quad_blur(dec, quad_sigma):
    """the image the threshold, the segmentation and the quad fit read, for the decimated image dec"""
    dec = np.ascontiguousarray(dec, dtype=np.uint8)
    k = blur_taps(quad_sigma)
    if len(k) == 0:
        return dec.copy()
    blurred = np.ascontiguousarray(_filter_rows(np.ascontiguousarray(_filter_rows(dec, k).T), k).T)
    if quad_sigma > 0:
        return blurred
    return np.clip(2 * dec.astype(np.int32) - blurred.astype(np.int32), 0, 255).astype(np.uint8)
