"""quad_sigma without a GPU: the library's taps (asl_blur_taps, a host function) against the NumPy statement
tests/blur_ref.py, and the properties of that statement."""
import numpy as np
import pytest

import blur_ref
from aprilslam_amd import _lib

SIGMAS = (0.3, 0.4, 0.5, 0.8, 1.0, 1.25, 1.5, 1.9, 2.5, 3.9)


@pytest.mark.parametrize("s", [sg * sign for sg in SIGMAS for sign in (1, -1)])
def test_library_taps_are_the_statements(s):
    assert np.array_equal(_lib.blur_taps(s), blur_ref.blur_taps(s)), s


def test_hand_checked_taps():
    assert blur_ref.blur_taps(0.8).tolist() == [60, 133, 60]
    assert _lib.blur_taps(0.8).tolist() == [60, 133, 60]
    assert len(blur_ref.blur_taps(0.4)) == 0 and len(_lib.blur_taps(0.4)) == 0
    assert len(blur_ref.blur_taps(0.5)) == 3 and len(_lib.blur_taps(0.5)) == 3
    assert len(_lib.blur_taps(0.0)) == 0
    assert [len(blur_ref.blur_taps(s)) for s in SIGMAS] == [0, 0, 3, 3, 5, 5, 7, 7, 11, 15]
    for s in SIGMAS:  # symmetric, and a little under 256 in sum
        k = blur_ref.blur_taps(s).astype(int)
        assert np.array_equal(k, k[::-1])
        assert len(k) == 0 or 256 - len(k) <= k.sum() <= 255


@pytest.mark.parametrize("s", [4.0, -4.0, 17.0, float("nan"), float("inf"), float("-inf")])
def test_refused_sigmas(s):
    with pytest.raises(_lib.AslError):
        _lib.blur_taps(s)


def test_taps_need_room():
    import ctypes as C
    L = _lib.load()
    buf = (C.c_uint8 * 15)(*([7] * 15))
    ksz = C.c_int(-5)
    assert L.asl_blur_taps(1.9, buf, 6, C.byref(ksz)) != 0     # 7 taps
    assert list(buf) == [7] * 15 and ksz.value == -5           # nothing written
    assert L.asl_blur_taps(1.9, buf, 7, C.byref(ksz)) == 0 and ksz.value == 7
    assert list(buf)[:7] == blur_ref.blur_taps(1.9).tolist() and list(buf)[7:] == [7] * 8
    assert L.asl_blur_taps(0.4, None, 0, C.byref(ksz)) == 0 and ksz.value == 0   # off needs no room


@pytest.mark.parametrize("s", [0.8, 1.25, 1.9, 3.9])
def test_constant_image(s):
    k = blur_ref.blur_taps(s)
    r = len(k) // 2
    h, w = 2 * len(k) + 5, 2 * len(k) + 8
    for c in (0, 1, 77, 200, 255):
        out = blur_ref.quad_blur(np.full((h, w), c, np.uint8), s)
        once = (c * int(k.sum())) >> 8
        inner = (once * int(k.sum())) >> 8   # both passes filter here
        want = np.full((h, w), c, np.int64)
        want[:, r:w - r - 1] = once          # rows pass
        want[r:h - r - 1, :] = (want[r:h - r - 1, :] * int(k.sum())) >> 8   # columns pass, over the rows pass's output
        assert np.array_equal(out, want)
        assert (out[r:h - r - 1, r:w - r - 1] == inner).all()
        # the copied border: r pixels at the left and top, r + 1 at the right and bottom
        assert (out[:r, :r] == c).all() and (out[h - r - 1:, w - r - 1:] == c).all()
        assert (out[:r, w - r - 1:] == c).all() and (out[h - r - 1:, :r] == c).all()
        if c >= 2:
            assert (out[r, r:w - r - 1] < c).all() and (out[h - r - 2, r:w - r - 1] < c).all()
            assert (out[r:h - r - 1, r] < c).all() and (out[r:h - r - 1, w - r - 2] < c).all()


@pytest.mark.parametrize("s", [0.8, -0.8, 1.9, 3.9])
def test_narrow_images_come_back_unchanged(s):
    ksz = len(blur_ref.blur_taps(s))
    rng = np.random.default_rng(int(abs(s) * 10))
    for h, w in ((ksz, ksz), (ksz - 1, ksz), (ksz, ksz - 2), (1, 1)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        assert np.array_equal(blur_ref.quad_blur(img, s), img)
    # narrow in one direction only: that direction is copied, the other is filtered
    img = rng.integers(0, 256, (ksz, 4 * ksz), dtype=np.uint8)
    out = blur_ref.quad_blur(img, abs(s))
    assert np.array_equal(out, blur_ref._filter_rows(img, blur_ref.blur_taps(s)))
    assert not np.array_equal(out, img)
    # one pixel wider than the kernel: exactly one filtered pixel per line
    img = rng.integers(1, 256, (ksz + 1, ksz + 1), dtype=np.uint8)
    out = blur_ref.quad_blur(img, abs(s))
    r = ksz // 2
    changed = out != img
    changed[r, :] = False
    changed[:, r] = False
    assert not changed.any()


def test_filter_is_the_plain_sum():
    """the vectorised statement against the definition written out pixel by pixel"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 17), dtype=np.uint8)
    for s in (0.8, 1.25, 1.9):
        k = blur_ref.blur_taps(s).astype(int)
        r = len(k) // 2

        def line(v):
            o = list(v)
            for i in range(r, len(v) - r - 1):
                o[i] = sum(int(k[j]) * int(v[i - r + j]) for j in range(len(k))) >> 8
            return o
        hor = np.array([line(row) for row in img])
        ver = np.array([line(col) for col in hor.T]).T
        assert np.array_equal(blur_ref.quad_blur(img, s), ver)
        assert np.array_equal(blur_ref.quad_blur(img, -s), np.clip(2 * img.astype(int) - ver, 0, 255))


def test_sharpening_clips_at_both_ends():
    img = np.zeros((24, 24), np.uint8)
    img[:, 12:] = 255
    for s in (-0.8, -1.9):
        out = blur_ref.quad_blur(img, s)
        soft = blur_ref.quad_blur(img, -s)
        assert out.dtype == np.uint8
        r = len(blur_ref.blur_taps(s)) // 2
        row = 12
        # black side of the edge: 2 * 0 - blurred < 0 -> 0; white side: 2 * 255 - blurred > 255 -> 255
        assert (soft[row, 12 - r:12] > 0).all() and (out[row, 12 - r:12] == 0).all()
        assert (soft[row, 12:12 + r] < 255).all() and (out[row, 12:12 + r] == 255).all()
        assert set(np.unique(out)) == {0, 255}
    # a mid-gray step does overshoot without clipping
    img = np.full((24, 24), 100, np.uint8)
    img[:, 12:] = 150
    out = blur_ref.quad_blur(img, -0.8).astype(int)
    assert out[12, 11] < 100 and out[12, 12] > 150
