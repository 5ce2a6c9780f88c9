"""CPU checks of the PnP statement (pnp_ref.py) and of the cases the GPU test runs (pnp_cases.py): the statement against
the C oracle class by class -- the measured spread is the basis of the GPU tolerance --, every case at the edge it is named
for, and the GPU test's comparison rejecting poses that are slightly wrong."""
import numpy as np
import pytest

import oracle_lib as O
import pnp_cases as PC
import pnp_ref as PR


@pytest.mark.parametrize("name", list(PC.SPREAD))
def test_statement_agrees_with_the_oracle_within_the_recorded_spread(name):
    worst = 0.0
    for cls, lens in PC.pose_classes():
        if cls != name:
            continue
        st, orc = PC.statement(cls, lens), PC.oracle(cls, lens)
        assert st[3].all() and orc[3].all(), (cls, lens)
        e = PC.pose_error(st[2], orc[2])
        print("%s / %s: spread %.3g (tag %d)" % (cls, lens, e.max(), e.argmax()))
        worst = max(worst, float(e.max()))
    assert worst <= PC.SPREAD[name] <= PC.SPREAD_CAP, (name, worst)
    assert PC.tolerance(name) == max(10 * PC.SPREAD[name], 1e-9) <= 1e-6


def test_classes_are_what_the_issue_of_each_says():
    for name, (T, noise, _) in PC.POSE_CLASSES.items():
        assert len(T) <= 128
        for lens in PC.LENSES:
            c = PC.class_corners(name, lens)
            assert c.dtype == np.float32 and c.shape == (len(T), 4, 2) and np.isfinite(c).all()
    assert PC.mixed37("all5").shape == (37, 4, 2) and len(PC.mirror_corners()) == PC.MIRROR_N + PC.N_FRONTAL
    # the barrel lens at the frame's corner: five sweeps leave the undistortion short of its fixed point
    cam = PR.camera(PC.K, PC.LENSES["barrel"])
    c = PC.class_corners(PC.BARREL_CORNER, "barrel").astype(np.float64).reshape(-1, 2)
    xy = PR.undistort(cam, c)
    back = PR.LR.project(cam, np.c_[xy, np.ones(len(xy))])
    assert np.abs(back - c).max() > 1e-3, np.abs(back - c).max()
    mid = PC.class_corners("tilts", "barrel").astype(np.float64).reshape(-1, 2)
    xy = PR.undistort(cam, mid)
    assert np.abs(PR.LR.project(cam, np.c_[xy, np.ones(len(xy))]) - mid).max() < np.abs(back - c).max()


@pytest.mark.parametrize("lens", list(PC.LENSES))
def test_half_turns_take_the_branch_they_are_named_for(lens):
    rv, tv, T, ok, recs = PC.statement("half_turns", lens)
    n = PC.N_FRONTAL
    s = np.array([r["s"] for r in recs])
    c = np.array([r["c"] for r in recs])
    assert (s[:2 * n] < PR.HALF_TURN_SIN).all() and (c[:2 * n] < 0).all()      # frontal, tilted by TILT_BELOW: the half-turn branch
    assert (np.abs(s[n:2 * n] - PC.TILT_BELOW) < 0.1 * PC.TILT_BELOW).all()    # ... and not by the rounding's grace
    assert (s[2 * n:3 * n] > PR.HALF_TURN_SIN).all() and (np.abs(s[2 * n:3 * n] - PC.TILT_ABOVE) < 0.1 * PC.TILT_ABOVE).all()
    assert s[3 * n] < PR.HALF_TURN_SIN and c[3 * n] > 0 and np.array_equal(rv[3 * n], np.zeros(3))   # R = I: rvec is 0
    assert np.array_equal(T[3 * n, :3, :3], np.eye(3))
    for i in range(len(T)):
        assert np.abs(PR.rotation_of(rv[i]) - T[i, :3, :3]).max() == 0
    # both signs of R[0][1] and both orderings of |rx| and |ry| among the frontal tags
    R01 = T[:n, 0, 1]
    assert (R01 > 0.1).any() and (R01 < -0.1).any()
    assert (np.abs(rv[:n, 0]) < np.abs(rv[:n, 1])).any() and (np.abs(rv[:n, 0]) > np.abs(rv[:n, 1])).any()
    assert np.abs(np.sqrt((rv[:2 * n] ** 2).sum(axis=1)) - np.pi).max() < 1e-5


def test_rot_to_rvec_inverts_rotation_of_on_both_sides_of_the_branch():
    rng = np.random.default_rng(3)
    for th in (0.0, 0.3, 2.0, np.pi - 1e-3, np.pi - 3e-5, np.pi - 2e-6, np.pi):
        for _ in range(8):
            a = rng.normal(size=3)
            a /= np.sqrt(a @ a)
            R = PR.rotation_of(a * th)
            r = PR.rot_to_rvec(R)
            # inside the half-turn branch the axis comes from the diagonal: exact only at pi, off by the distance to pi before it
            lim = 1e-9 if th < np.pi - 1e-4 or th == np.pi else 4 * (np.pi - th)
            assert np.abs(PR.rotation_of(r) - R).max() < lim, (th, a)


def test_mirror_class_decides_between_the_minima():
    rv, tv, T, ok, recs = PC.mirror_statement()
    n = PC.MIRROR_N
    assert ok.all()
    won = np.array([r["mirrored"] for r in recs])
    band = PC.mirror_band(recs)
    print("mirror: the mirrored start wins %d of %d, %d within %g of each other" % (won[:n].sum(), n, band[:n].sum(), PC.MIRROR_BAND))
    assert 5 <= won[:n].sum() <= n // 2
    assert band[:n].sum() <= PC.MIRROR_BAND_SHARE * n
    assert all(np.isfinite(r["cost_mirror"]) and r["sn"] > PR.MIRROR_SIN for r in recs[:n])
    # the frontal tags have no second pose: |n x m| <= 1e-6, no mirrored solve
    assert all(r["sn"] <= PR.MIRROR_SIN and r["T_mirror"] is None and not r["mirrored"] for r in recs[n:])
    # the choice is the lower cost, and cost() of the returned pose is that cost
    cam = PR.camera(PC.K, None)
    c = PC.mirror_corners()
    for i in (0, 1, int(np.flatnonzero(won)[0])):
        r = recs[i]
        assert r["mirrored"] == (r["cost_mirror"] < r["cost_plain"])
        assert abs(PR.cost(T[i], c[i], cam) - min(r["cost_plain"], r["cost_mirror"])) < 1e-9 * (1 + r["cost_plain"])
    # off: the plain minimum, whatever the mirrored one would cost
    off = PR.solve_pnp(c[:8], PC.K, None, PC.TAG)
    assert all(np.array_equal(off[2][i], recs[i]["T_plain"]) for i in range(8))


def test_failures_fail_in_the_oracle_and_in_the_statement():
    names, c = PC.failures()
    assert len(names) == 6
    orv, otv, oT, ook = O.solve_pnp(c, PC.K, np.zeros(0), PC.TAG)
    rv, tv, T, ok = PR.solve_pnp(c, PC.K, None, PC.TAG)
    assert not ook.any() and not ok.any(), (names, ook, ok)
    assert not rv.any() and not tv.any() and not T.any()
    for on in (False, True):
        assert not PR.solve_pnp(c, PC.K, np.zeros(4), PC.TAG, both_minima=on)[3].any()
    # five leave at the homography's two checks; LATE_FAILURE passes them with a non-finite homography and fails at the end
    cam, h = PR.camera(PC.K, None), PR.LR.half_size(PC.TAG)
    for name, ci in zip(names, c):
        with np.errstate(all="ignore"):
            H = PR.homography(PR.undistort(cam, ci.astype(np.float64)), h)
        assert (H is not None and not np.isfinite(H).all()) if name == PC.LATE_FAILURE else H is None, name
    # the path-sensitive inputs are finite float32, and through a lens the oracle does return a pose for each
    p = PC.path_sensitive()
    assert np.isfinite(p).all() and O.solve_pnp(p, PC.K, PC.LENSES["all5"], PC.TAG)[3].all()
    # through a lens every input that stays exactly degenerate still fails in both
    lens_ok_o = O.solve_pnp(c, PC.K, PC.LENSES["all5"], PC.TAG)[3]
    lens_ok_s = PR.solve_pnp(c, PC.K, PC.LENSES["all5"], PC.TAG)[3]
    assert np.array_equal(lens_ok_o, lens_ok_s) and not lens_ok_o[[0, 1, 4, 5]].any()


def _turned(res, angle):
    rv, tv, T, ok = [np.array(a) for a in res[:4]]
    Q = PR.rotation_of(np.array([0.0, 0.0, angle]))
    for i in range(len(T)):
        T[i, :3, :3] = Q @ T[i, :3, :3]   # not rebuilt from rvec: rot_to_rvec takes a turn of 1e-5 off the identity for none
        rv[i] = PR.rot_to_rvec(T[i, :3, :3])
    return rv, tv, T, ok


@pytest.mark.parametrize("name,lens", [("tilts", "none"), ("noisy", "barrel"), ("half_turns", "all5"), ("near_far", "k3")])
def test_the_comparison_of_the_gpu_test_is_sharp(name, lens):
    ref = PC.statement(name, lens)
    tol = PC.tolerance(name)
    assert PC.check_poses(ref[:4], ref[:4], tol) == []
    assert PC.check_poses(ref[:4], PC.oracle(name, lens), tol) == []
    # every pose turned by 1e-5 rad about the optical axis
    bad = PC.check_poses(_turned(ref, 1e-5), ref[:4], tol)
    assert sum("pose off" in b for b in bad) == len(ref[2]), bad[:3]
    # one pair of corners swapped in one tag
    c = PC.class_corners(name, lens).copy()
    c[1, [0, 1]] = c[1, [1, 0]]
    bad = PC.check_poses(PR.solve_pnp(c, PC.K, PC.LENSES[lens], PC.TAG), ref[:4], tol)
    assert bad and all(b.startswith("tag 1:") or b.startswith("ok differs at [1]") for b in bad), bad
    # one rvec with its sign flipped, away from pi (at pi the two signs are the same rotation, and are let through)
    th = np.sqrt((ref[0] ** 2).sum(axis=1))
    i = int(np.flatnonzero((th > 0.1) & (th < np.pi - 0.05))[0]) if ((th > 0.1) & (th < np.pi - 0.05)).any() else None
    if i is not None:
        rv = np.array(ref[0])
        rv[i] = -rv[i]
        bad = PC.check_poses((rv, ref[1], ref[2], ref[3]), ref[:4], tol)
        assert any(b.startswith("tag %d: rvec off" % i) for b in bad) and any(b.startswith("tag %d: T is not" % i) for b in bad), bad
    # a failed record that is not zero, and an ok that differs
    T = np.array(ref[2])
    ok = np.array(ref[3])
    ok[0] = False
    assert PC.check_poses((ref[0], ref[1], T, ok), ref[:4], tol) == ["ok differs at [0]"]
    assert PC.check_poses((ref[0], ref[1], T, ok), (ref[0], ref[1], ref[2], ok), tol) == ["tag 0: ok = 0 but the record is not zero"]


def test_the_sign_flip_case_exists():
    """the rvec comparison needs poses away from pi to bite: the tilted classes have them"""
    th = np.sqrt((PC.statement("tilts", "none")[0] ** 2).sum(axis=1))
    assert ((th > 0.1) & (th < np.pi - 0.05)).sum() >= 16
