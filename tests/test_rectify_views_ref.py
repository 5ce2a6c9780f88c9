"""The statement of rectification into rotated pinhole views (tests/rectify_views_ref.py) against what it must agree with:
its written-out arctangent against np.arctan2, its projection against its own inverse, its Brown path against
rectify_ref.py, its view mapping against the rig camera the view becomes, the product's point maps against it, and the
recorded figures of tests/rectify_views_cases.py against a fresh measurement.  No GPU."""
import numpy as np
import pytest

import rectify_ref as RR
import rectify_views_cases as VC
import rectify_views_ref as VR
from aprilslam_amd import rectify
from aprilslam_amd.rectify import ViewSet

FISH_K = np.array([[193.0, 0.0, 320.3], [0.0, 191.0, 239.6], [0.0, 0.0, 1.0]])
FISH_DIST = np.array([-0.01, 0.003, -0.0005, 0.00002])
BROWN_DIST = np.array([-0.2, 0.05, 0.01, -0.02, 0.03])


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def test_arctangent_within_2_ulp_of_numpys():
    """a million random (r >= 0, Z) over 120 binades of ratio, and the edges"""
    rng = np.random.default_rng(20251021)
    n = 1000000
    r = np.abs(rng.standard_normal(n)) * np.exp2(rng.integers(-30, 31, n))
    Z = rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))
    worst = float(ulps(VR.atan2_pos(r, Z), np.arctan2(r, Z)).max())
    print("random pairs: %.2f ulp" % worst)
    assert worst <= 2
    r = rng.uniform(0, 2, n)
    Z = rng.uniform(-2, 2, n)
    assert ulps(VR.atan2_pos(r, Z), np.arctan2(r, Z)).max() <= 2
    e = 2.0 ** 60
    edges = [(0.0, 1.0), (0.0, 3e-300), (0.0, -1.0), (0.0, -e), (1.0, 0.0), (1e-300, 0.0), (e, 0.0), (0.0, 0.0),
             (1.0, -1.0), (1.0, 1.0), (1.0, -1e-300), (1.0, 1e-300),
             (e, 1.0), (1.0, e), (e, -1.0), (1.0, -e), (1.0 / e, 1.0), (1.0, 1.0 / e), (1.0 / e, -1.0), (1.0, -1.0 / e), (3.7 * e, 1.3), (1.3, -3.7 * e),
             (0.4375, 1.0), (0.6875, 1.0), (1.1875, 1.0), (2.4375, 1.0), (0.4375, -1.0), (2.4375, -1.0)]
    for r, Z in edges:
        got, want = float(VR.atan2_pos(r, Z)), float(np.arctan2(r, Z))
        assert 0 <= got <= np.pi
        assert (got == want) if want == 0 else ulps(got, want) <= 2, (r, Z, got, want)
    # the thresholds of the reduction from below and above: the pieces join within the bound
    for c in (0.4375, 0.6875, 1.1875, 2.4375):
        t = np.array([np.nextafter(c, 0), c, np.nextafter(c, 4)])
        assert ulps(VR.atan2_pos(t, np.ones(3)), np.arctan2(t, np.ones(3))).max() <= 2


def test_project_and_unproject_round_trip_out_to_100_degrees():
    th, ph = np.meshgrid(np.radians(np.linspace(0, 100, 41)), np.radians(np.arange(0, 360, 15)))
    rays = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1)
    for dist in (None, FISH_DIST):
        uv = VR.fisheye_project(rays, FISH_K, dist)
        back = VR.fisheye_unproject(uv[..., 0], uv[..., 1], FISH_K, dist)
        assert np.abs(np.linalg.norm(back, axis=-1) - 1).max() < 1e-12
        again = VR.fisheye_project(back, FISH_K, dist)
        print("round trip: %.3g px" % np.abs(again - uv).max())
        assert np.abs(again - uv).max() <= 1e-9
        assert np.abs(back - rays).max() <= 1e-9 / 190          # the same 1e-9 px as an angle
    # the pixel a view samples is the projection of that pixel's ray
    Kn, R = ViewSet.fan(FISH_K, FISH_DIST, "fisheye", 3, 90, (64, 48)).views[2]
    xs, ys = np.meshgrid(np.arange(64) + 0.5, np.arange(48) + 0.5)
    u, v = VR.source_coords(xs, ys, FISH_K, FISH_DIST, VR.LENS_FISHEYE, Kn, R)
    dv = np.stack([(xs - Kn[0, 2]) / Kn[0, 0], (ys - Kn[1, 2]) / Kn[1, 1], np.ones_like(xs)], axis=-1)
    assert np.abs(np.stack([u, v], axis=-1) - VR.fisheye_project(dv @ R.T, FISH_K, FISH_DIST)).max() <= 1e-9


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("n_dist", [0, 4, 5])
def test_identity_view_under_brown_is_rectify_ref(n_dist, ch):
    rng = np.random.default_rng(n_dist + ch)
    src = rng.integers(0, 256, (19, 37) + ((3,) if ch == 3 else ()), dtype=np.uint8)
    K = np.array([[33.3, 0.0, 18.8], [0.0, 36.6, 9.1], [0.0, 0.0, 1.0]])
    Kn = np.array([[25.0, 0.0, 15.8], [0.0, 27.0, 10.7], [0.0, 0.0, 1.0]])
    dist = None if n_dist == 0 else BROWN_DIST[:n_dist]
    got = VR.rectify_views(src, K, dist, VR.LENS_BROWN, [(Kn, np.eye(3)), (Kn, None)], 33, 21, fill=77)
    want = RR.rectify(src, K, dist, Kn, 33, 21, fill=77)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    assert (want == 77).any() and len(np.unique(want)) > 50
    xs, ys = np.meshgrid(np.arange(33) + 0.5, np.arange(21) + 0.5)
    u, v = VR.source_coords(xs, ys, K, dist, VR.LENS_BROWN, Kn, np.eye(3))
    u0, v0 = RR._source_coords(xs, ys, K, dist, Kn)
    assert np.array_equal(u, u0) and np.array_equal(v, v0)


def test_the_lens_cases_that_give_fill():
    src = np.full((48, 64), 200, dtype=np.uint8)
    K = np.array([[20.0, 0.0, 32.0], [0.0, 20.0, 24.0], [0.0, 0.0, 1.0]])   # 20 px/rad: the frame holds 90 degrees and more
    Kn = np.array([[16.0, 0.0, 16.0], [0.0, 16.0, 12.0], [0.0, 0.0, 1.0]])
    R = rectify._axis_rotation("y", np.radians(120.0))
    xs, ys = np.meshgrid(np.arange(32) + 0.5, np.arange(24) + 0.5)
    Z = R[2, 0] * (xs - 16.0) / 16.0 + R[2, 1] * (ys - 12.0) / 16.0 + R[2, 2]
    assert (Z < 0).any() and (Z > 0).any()
    brown = VR.rectify_views(src, K, None, VR.LENS_BROWN, [(Kn, R)], 32, 24, fill=9)[0]
    assert (brown[Z <= 0] == 9).all()
    fish = VR.rectify_views(src, K, None, VR.LENS_FISHEYE, [(Kn, R)], 32, 24, fill=9)[0]
    assert (fish[Z < 0] == 200).any()                      # behind the camera plane and still an ordinary ray
    cut = VR.rectify_views(src, K, None, VR.LENS_FISHEYE, [(Kn, R)], 32, 24, fill=9, theta_max=np.radians(100.0))[0]
    dv = np.stack([(xs - 16.0) / 16.0, (ys - 12.0) / 16.0, np.ones_like(xs)], axis=-1) @ R.T
    th = np.arctan2(np.hypot(dv[..., 0], dv[..., 1]), dv[..., 2])
    clear = np.abs(th - np.radians(100.0)) > 1e-9
    assert np.array_equal((cut == 9)[clear], ((th > np.radians(100.0)) | (fish == 9))[clear])
    assert (cut == 9).any() and (cut == 200).any()
    with pytest.raises(ValueError):
        VR.rectify_views(src, K, None, VR.LENS_FISHEYE, [(Kn, R)], 32, 24, theta_max=4.0)
    with pytest.raises(ValueError):
        VR.rectify_views(src, K, BROWN_DIST, VR.LENS_FISHEYE, [(Kn, R)], 32, 24)


def test_the_axis_pixel_samples_the_principal_point():
    src = np.random.default_rng(5).integers(0, 256, (48, 64), dtype=np.uint8)
    K = np.array([[40.0, 0.0, 30.0], [0.0, 40.0, 20.0], [0.0, 0.0, 1.0]])      # (cx, cy) on a corner of four pixels
    Kn = np.array([[30.0, 0.0, 7.5], [0.0, 30.0, 5.5], [0.0, 0.0, 1.0]])
    u, v = VR.source_coords(7.5, 5.5, K, FISH_DIST, VR.LENS_FISHEYE, Kn, np.eye(3))
    assert (float(u), float(v)) == (30.0, 20.0)
    out = VR.rectify_views(src, K, FISH_DIST, VR.LENS_FISHEYE, [(Kn, np.eye(3))], 16, 12)[0]
    assert out[5, 7] == int(np.floor(src[19:21, 29:31].astype(np.float64).sum() / 4 + 0.5))


def test_a_view_maps_as_its_rig_camera_projects():
    """the pixel of a view a ray lands on = the projection of the ray through the matching RigCamera of ViewSet.rig()"""
    vs = ViewSet.fan(FISH_K, FISH_DIST, "fisheye", 3, 90, (640, 480), step_deg=60)
    rig = vs.rig()
    assert len(rig) == 3 and all(len(c.dist) == 0 for c in rig.cameras)
    pts = np.random.default_rng(3).uniform([0, 0], [640, 480], (500, 2))
    for v, (Kn, R) in enumerate(vs.views):
        cam = rig.cameras[v]
        assert np.array_equal(cam.K, Kn) and np.array_equal(cam.T_cam_rig[:3, :3], R.T) and not cam.T_cam_rig[:3, 3].any()
        u, w_ = VR.source_coords(pts[:, 0], pts[:, 1], FISH_K, FISH_DIST, VR.LENS_FISHEYE, Kn, R)
        rays = VR.fisheye_unproject(u, w_, FISH_K, FISH_DIST)             # in the rig frame = the source camera's
        P = rays @ cam.T_cam_rig[:3, :3].T + cam.T_cam_rig[:3, 3]
        proj = np.stack([cam.K[0, 0] * P[:, 0] / P[:, 2] + cam.K[0, 2], cam.K[1, 1] * P[:, 1] / P[:, 2] + cam.K[1, 2]], axis=-1)
        print("view %d: %.3g px" % (v, np.abs(proj - pts).max()))
        assert np.abs(proj - pts).max() <= 1e-9
        # the product's two point maps say the same
        assert np.abs(vs.distort_points(v, pts) - np.stack([u, w_], axis=-1)).max() <= 1e-9
        assert np.abs(vs.undistort_points(v, np.stack([u, w_], axis=-1)) - pts).max() <= 1e-9
    assert np.isnan(vs.undistort_points(0, vs.distort_points(2, np.array([[600.0, 240.0]])))).all()   # behind the left view


def test_fan():
    vs = ViewSet.fan(FISH_K, FISH_DIST, "fisheye", 3, 90, (640, 480))
    assert [round(float(np.degrees(np.arctan2(R[0, 2], R[2, 2]))), 9) for _, R in vs.views] == [-90.0, 0.0, 90.0]   # abutting
    Kn = vs.views[0][0]
    assert abs(Kn[0, 0] - 320.0) < 1e-9 and Kn[0, 0] == Kn[1, 1] and (Kn[0, 2], Kn[1, 2]) == (320.0, 240.0)
    # the right edge of a view and the left edge of the next are the same rays
    a = vs.distort_points(0, np.array([[640.0, 100.0], [640.0, 400.0]]))
    b = vs.distort_points(1, np.array([[0.0, 100.0], [0.0, 400.0]]))
    assert np.abs(a - b).max() < 1e-9
    up = ViewSet.fan(FISH_K, None, "fisheye", 2, 60, (64, 48), axis="x")
    assert up.distort_points(1, np.array([[32.0, 24.0]]))[0, 1] > FISH_K[1, 2] > up.distort_points(0, np.array([[32.0, 24.0]]))[0, 1]


def test_save_and_load(tmp_path):
    vs = ViewSet.fan(FISH_K, FISH_DIST, "fisheye", 3, 90, (640, 480), step_deg=60, theta_max=1.7, fill=3)
    vs.save(str(tmp_path / "views.npz"))
    got = ViewSet.load(str(tmp_path / "views.npz"))
    assert got.records().tobytes() == vs.records().tobytes() and np.array_equal(got.K, vs.K) and np.array_equal(got.dist, vs.dist)
    assert (got.model, got.size, got.theta_max, got.fill) == (vs.model, vs.size, vs.theta_max, vs.fill)


def test_distort_points_with_todays_arguments_is_bit_identical():
    pts = np.random.default_rng(0).uniform(-50, 700, (4, 250, 2))
    K = np.array([[500.0, 0.0, 320.5], [0.0, 510.0, 240.25], [0.0, 0.0, 1.0]])
    Kn = np.array([[400.0, 0.0, 310.0], [0.0, 410.0, 250.0], [0.0, 0.0, 1.0]])
    for dist in (None, BROWN_DIST[:4], BROWN_DIST):
        for k_new in (None, Kn):
            assert rectify.distort_points(pts, K, dist, k_new).tobytes() == RR.distort_points(pts, K, dist, k_new).tobytes()
            assert rectify.distort_points(pts, K, dist, K_new=k_new).tobytes() == RR.distort_points(pts, K, dist, k_new).tobytes()
    with pytest.raises(ValueError):
        rectify.distort_points(pts, K, BROWN_DIST[:3])


def test_tag_detector_refuses_a_fisheye_without_rectification():
    from aprilslam_amd.tag_detector import TagDetector
    params = {"camera_matrix": FISH_K, "dist_coeffs": FISH_DIST}
    with pytest.raises(ValueError):
        TagDetector(params, lens_model="fisheye")
    with pytest.raises(ValueError):
        TagDetector(params, lens_model="equidistant", rectify=True)


def test_the_scene_needs_the_views():
    """on the raw fisheye frame the oracle misses the tag at -78 degrees (and the corners it finds are those of bent edges,
    of no use to a pinhole PnP); on the three views it finds all six, two per view, hamming 0 (asserted in measure())"""
    import oracle_lib as O
    from aprilslam_amd.families import get_family
    raw = [d["id"] for d in O.detect_bgr(VC.fisheye_frame(), get_family())]
    print("raw fisheye frame: ids", raw)
    assert 0 not in raw and set(raw) < set(VC.ground_truth())
    VC.measure()


@pytest.mark.parametrize("name", sorted(VC.recorded()))
def test_recorded_figures_are_the_measured_ones(name):
    """the bounds the GPU tests use stand on these figures: each is what the oracle and the statements give now, rounded up"""
    got, (measured, bound) = VC.measure()[name], VC.recorded()[name]
    print("%s: measured %.6g, recorded %.6g, bound %.6g" % (name, got, measured, bound))
    assert got <= measured <= 1.001 * got and bound == 2 * measured
