"""The statement of lens rectification (tests/rectify_ref.py) against what it must do by construction, against synth's own
lens model, and -- through the CPU oracle detector -- against the renderer's pinhole image of the same scene.  No GPU."""
import numpy as np
import pytest

import calib_cases as CC
import rectify_cases as RC
import rectify_ref as RR
from aprilslam_amd import rectify, synth


def small_camera(w, h):
    return np.array([[29.5, 0.0, 0.5 * w + 0.3], [0.0, 31.25, 0.5 * h - 0.4], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(5)
    gray = rng.integers(0, 256, (19, 37), dtype=np.uint8)
    bgr = rng.integers(0, 256, (19, 37, 3), dtype=np.uint8)
    return gray, bgr


def test_bgr_gray_is_the_detectors_formula(images):
    import oracle_lib as O
    assert np.array_equal(RR.bgr_gray(images[1]), O.bgr2gray(images[1]))
    every = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(0, 256, 3), np.arange(0, 256, 7), indexing="ij"), -1).astype(np.uint8)
    assert np.array_equal(RR.bgr_gray(every), O.bgr2gray(every.reshape(1, -1, 3))[0].reshape(every.shape[:3]))


@pytest.mark.parametrize("n_dist", [0, 4, 5])
def test_identity(images, n_dist):
    """no lens, K_new = K, the same size: the source itself, and the gray conversion for BGR, byte for byte at 37 x 19"""
    gray, bgr = images
    K = small_camera(37, 19)
    dist = None if n_dist == 0 else np.zeros(n_dist)
    for K_new in (None, K):
        assert np.array_equal(RR.rectify(gray, K, dist, K_new, 37, 19), gray)
        assert np.array_equal(RR.rectify(bgr, K, dist, K_new, 37, 19), RR.bgr_gray(bgr))


@pytest.mark.parametrize("fill", [0, 200])
def test_pure_shift(images, fill):
    """cx' = cx - 3: output column x shows source column x + 3; the last 3 columns look past the source"""
    gray, bgr = images
    K = small_camera(37, 19)
    Kn = K.copy()
    Kn[0, 2] -= 3
    for src, want in ((gray, gray), (bgr, RR.bgr_gray(bgr))):
        out = RR.rectify(src, K, None, Kn, 37, 19, fill=fill)
        assert np.array_equal(out[:, :34], want[:, 3:])
        assert (out[:, 34:] == fill).all()


def test_nan_and_outside_give_fill(images):
    gray, _ = images
    K = small_camera(37, 19)
    out = RR.rectify(gray, K, np.array([8.0, 0, 0, 0]), None, 37, 19, fill=7)  # k1 = +8: only the centre stays inside
    assert (out[:, :6] == 7).all() and (out[:, -6:] == 7).all() and (out[8:11, 17:20] != 7).any()
    assert (RR.rectify(gray, K, np.array([1e308, 1e308, 0, 0, 1e308]), None, 37, 19, fill=9) == 9).sum() >= out.size - 4


def test_round_trip_through_synths_inverse():
    """distort_points, then synth.undistort_normalized and K_new, is the identity to 1e-9 px under CC.WEBCAM_DIST.
    synth's inverse is 8 fixed-point steps that contract by about q = 3 |k1| r^2 each, from a first error of about |k1| r^3
    (r: the normalised radius): f |k1| r^3 q^8 px is left.  That is 5e-11 px at r = 0.36 (150 px from the principal point at
    f = 415.7) and 3e-8 px at r = 0.5, so the points are taken within 150 px, where the inverse has converged; further out the
    test would measure synth's iteration count, not distort_points."""
    K = synth.camera_matrix(CC.WEBCAM_W, CC.WEBCAM_H, CC.WEBCAM_FOV)
    Kn = K.copy()
    Kn[0, 0] *= 0.9
    Kn[1, 1] *= 0.85
    Kn[0, 2] += 4.25
    rng = np.random.default_rng(3)
    ang, rad = rng.uniform(0, 2 * np.pi, 500), 150.0 * np.sqrt(rng.uniform(0, 1, 500))
    src = np.stack([K[0, 2] + rad * np.cos(ang), K[1, 2] + rad * np.sin(ang)], axis=-1)   # where the points land in the source
    x, y = synth.undistort_normalized((src[:, 0] - K[0, 2]) / K[0, 0], (src[:, 1] - K[1, 2]) / K[1, 1], CC.WEBCAM_DIST)
    pts = np.stack([x * Kn[0, 0] + Kn[0, 2], y * Kn[1, 1] + Kn[1, 2]], axis=-1)           # rectified points that land there
    for fn in (RR.distort_points, rectify.distort_points):
        uv = fn(pts, K, CC.WEBCAM_DIST, Kn)
        assert np.hypot(uv[:, 0] - K[0, 2], uv[:, 1] - K[1, 2]).max() <= 150.0 + 1e-6
        xb, yb = synth.undistort_normalized((uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], CC.WEBCAM_DIST)
        back = np.stack([xb * Kn[0, 0] + Kn[0, 2], yb * Kn[1, 1] + Kn[1, 2]], axis=-1)
        err = np.abs(back - pts).max()
        print("round trip: %.3g px" % err)
        assert err <= 1e-9


def test_product_distort_points_is_the_statements():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-50, 700, (4, 25, 2))
    K, Kn = RC.cameras(RC.WIDE_FOV, RC.WIDE_FOV_NEW)
    for dist in (None, RC.WIDE_DIST[:4], RC.WIDE_DIST):
        for K_new in (None, Kn):
            assert np.array_equal(rectify.distort_points(pts, K, dist, K_new), RR.distort_points(pts, K, dist, K_new))


def test_against_the_renderers_model():
    """a scene rendered under the pinhole K_new, and the same scene rendered under K with a lens and rectified by the
    statement: the oracle finds the same ids (checked scene by scene in rectify_cases.measure), and its corners differ by
    no more than twice the largest difference over these scenes as it was measured and recorded."""
    got, rec = RC.measure(), RC.recorded()
    print("largest corner difference %.4f px, recorded %.4f px, bound %.4f px" % ((got["model_corner_px"],) + rec["model_corner_px"]))
    assert got["model_corner_px"] <= rec["model_corner_px"][1]


@pytest.mark.parametrize("name", sorted(RC.recorded()))
def test_recorded_figures_are_the_measured_ones(name):
    """the bounds the GPU tests use stand on these figures: each is what the oracle and the statement give now, rounded up"""
    got, (measured, bound) = RC.measure()[name], RC.recorded()[name]
    print("%s: measured %.6g, recorded %.6g, bound %.6g" % (name, got, measured, bound))
    assert got <= measured <= 1.001 * got and bound == 2 * measured


def test_wide_scene_needs_and_survives_rectification():
    """the wide-angle scene of the GPU test, chosen here: the oracle finds every tag of the scene in the statement-rectified
    frame, and the lens moves points of the frame by tens of pixels"""
    import oracle_lib as O
    from aprilslam_amd.families import get_family
    _, _, rect, gt, K, Kn, dist = RC.model_frames(RC.WIDE_SCENE[0])
    assert [d["id"] for d in O.detect_gray(rect, get_family())] == sorted(gt) and len(gt) == RC.N_TAGS
    corners = np.array([[0.0, 0.0], [RC.W, RC.H]])
    assert np.abs(RR.distort_points(corners, K, dist, None) - corners).max() > 30
