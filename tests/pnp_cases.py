"""Deterministic, seeded inputs of the per-tag PnP tests (test_pnp_ref.py on the CPU, test_gpu_pnp.py on the device).

The camera is synth.camera_matrix(1280, 720), the tag size 10.  A pose class is a list of camera<-tag poses; its corners
are the exact projections through one of LENSES (so every lens sees the same poses), rounded to float32, with the class's
pixel noise (drawn once, the same under every lens) added before the rounding.

A frontal tag faces the camera: its rotation is the half-turn about the in-plane axis a = (cos phi/2, sin phi/2, 0),
R = 2 a a^T - I, which turns the tag by phi in its plane.  A tilt about a itself by eps makes the angle pi + eps, so
|sin| = eps in rot_to_rvec: the two tilts of `half_turns` lie on either side of its 1e-5.  Every other tilt is about a
random in-plane axis.

SPREAD[class] is the largest difference between the NumPy statement (pnp_ref.py) and the C oracle (oracle/pnp_oracle.c)
over the class under every lens, as pose_error() measures it (rotation entries absolutely, the translation relative to
its length); test_pnp_ref.py checks that the constant covers what it measures, and tolerance() -- 10 x the spread, at
least 1e-9 -- is what the device is held to against either reference.  The factor 10: the device is a third rounding of
the same iteration, which can flip one more accept / reject decision than two roundings do.
"""
import numpy as np

import pnp_ref as PR
from aprilslam_amd import synth

K = synth.camera_matrix(1280, 720)
TAG = 10.0
LENSES = {
    "none": None,
    "zeros4": np.zeros(4),
    "all5": np.array([0.05, -0.02, 0.001, -0.0005, 0.01]),
    "tangential": np.array([0.0, 0.0, 0.01, -0.02]),
    "k3": np.array([0.0, 0.0, 0.0, 0.0, 0.02]),
    "barrel": np.array([-0.35, 0.15, 0.0, 0.0, -0.03]),
}
PHIS = (0, 30, 90, 150, 180, 210, 270, 330)
TILT_BELOW, TILT_ABOVE = 2e-6, 3e-5   # either side of rot_to_rvec's |sin| = 1e-5


def frontal(phi_deg):
    a = np.array([np.cos(np.radians(phi_deg) / 2), np.sin(np.radians(phi_deg) / 2), 0.0])
    return 2.0 * np.outer(a, a) - np.eye(3), a


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def half_turn_poses():
    """8 frontal at z = 100, 8 tilted by TILT_BELOW and 8 by TILT_ABOVE (about the half-turn's own axis) at z = 8, then
    R = I at z = 100.  The tilted ones are close: at z = 100 a tilt of eps moves a corner by f h^2 eps / z^2 = 2.2 eps
    pixels, 4e-6 px for TILT_BELOW, while float32 corners at these pixels are 3e-5 to 6e-5 px apart -- the rounded corners
    would be the frontal tag's, up to single flips worth |sin| = 1.4e-5 each, on the wrong side.  At z = 8 the same tilt
    moves a corner by 340 eps pixels and the rounding is worth |sin| = 2e-7.  They are also turned by 15 degrees more:
    below 1e-5 rot_to_rvec takes the signs of its axis from R[0][1] = sin phi and R[0][2] = -eps sin(phi / 2), which are
    exactly 0 at phi = 0 and 180 -- there the sign is the rounding's, and with it 2 eps of the rebuilt rotation (the
    statement and the oracle disagree by 4e-6 on those two tags)."""
    out = []
    for eps, z, turn in ((0.0, 100.0, 0), (TILT_BELOW, 8.0, 15), (TILT_ABOVE, 8.0, 15)):
        for phi in PHIS:
            R, a = frontal(phi + turn)
            out.append(pose(PR.rotation_of(a * eps) @ R, [0.0, 0.0, z]))
    out.append(pose(np.eye(3), [0.0, 0.0, 100.0]))   # the vertically mirrored corner order: rvec = 0
    return np.array(out)


N_FRONTAL = len(PHIS)


def tilted_poses(seed, n, tilt_deg, z_range, spread_xy=(0.35, 0.15)):
    """n poses tilted off frontal by tilt_deg = (lo, hi) about random in-plane axes, at depth z in z_range, the tag
    centre at most spread_xy * z off the axis"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R, _ = frontal(rng.uniform(0, 360))
        psi, tilt = rng.uniform(0, 2 * np.pi), np.radians(rng.uniform(*tilt_deg))
        z = rng.uniform(*z_range)
        t = [rng.uniform(-1, 1) * spread_xy[0] * z, rng.uniform(-1, 1) * spread_xy[1] * z, z]
        out.append(pose(PR.rotation_of(np.array([np.cos(psi), np.sin(psi), 0.0]) * tilt) @ R, t))
    return np.array(out)


def near_far_poses():
    near = tilted_poses(41, 8, (0, 30), (8, 8), spread_xy=(0.1, 0.1))
    far = tilted_poses(42, 8, (10, 60), (3000, 3000))
    return np.concatenate([near, far])


def frame_corner_poses():
    """tags that project near the frame's corners, where five undistortion sweeps of the barrel lens have not converged"""
    out = []
    for i, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
        for j, z in enumerate((60.0, 120.0)):
            P = tilted_poses(50 + 2 * i + j, 1, (10, 50), (z, z), spread_xy=(0, 0))[0]
            P[:3, 3] = [sx * 0.64 * z, sy * 0.34 * z, z]
            out.append(P)
    return np.array(out)


# class -> (poses, pixel noise sigma, noise seed)
POSE_CLASSES = {
    "half_turns": (half_turn_poses(), 0.0, 0),
    "tilts": (tilted_poses(11, 32, (10, 60), (40, 400)), 0.0, 0),
    "steep": (tilted_poses(12, 32, (60, 80), (40, 200)), 0.0, 0),
    "noisy": (tilted_poses(13, 32, (10, 60), (40, 150)), 0.3, 113),
    "near_far": (near_far_poses(), 0.0, 0),
}
BARREL_CORNER = "barrel_corner"   # frame_corner_poses under the barrel lens only

# largest |statement - oracle| of the class over every lens (pose_error): the measured value, rounded up to the next of
# 1, 2, 5 x 10^k.  test_pnp_ref.py measures it again and holds it under the constant, and the constant under SPREAD_CAP.
SPREAD = {
    "half_turns": 1e-9,     # measured 6.07e-10 (tangential lens, the frontal tag at phi = 0)
    "tilts": 5e-10,         # measured 3.09e-10 (tangential lens)
    "steep": 5e-11,         # measured 2.73e-11 (tangential lens, in the translation)
    "noisy": 1e-8,          # measured 9.05e-9 (tangential lens)
    "near_far": 1e-9,       # measured 5.89e-10 (no lens, a tag at z = 3000)
    BARREL_CORNER: 1e-14,   # measured 7.2e-15
}
SPREAD_CAP = 1e-7


def tolerance(name):
    return max(10 * SPREAD[name], 1e-9)


def project(T, dist, noise=0.0, seed=0):
    """float32 corners (n, 4, 2) of the poses T (n, 4, 4) through the lens dist"""
    cam = PR.camera(K, dist)
    c = np.array([PR.project_pose(Ti, cam, TAG) for Ti in T])
    if noise:
        c = c + np.random.default_rng(seed).normal(0, noise, c.shape)
    return c.astype(np.float32)


def class_corners(name, lens):
    if name == BARREL_CORNER:
        assert lens == "barrel"
        return project(frame_corner_poses(), LENSES["barrel"])
    T, noise, seed = POSE_CLASSES[name]
    return project(T, LENSES[lens], noise, seed)


def pose_classes():
    """every (class, lens) the pose comparisons run"""
    return [(n, l) for n in POSE_CLASSES for l in LENSES] + [(BARREL_CORNER, "barrel")]


# ---- inputs without a pose
LATE_FAILURE = "inf_corner"   # the one failure that runs the whole solve first (test_pnp_ref.py checks which exit each takes)


def failures():
    """(names, corners (6, 4, 2)): the inputs for which there is no pose, ok = 0"""
    sq = np.array([[600.0, 300.0], [700.0, 300.0], [700.0, 400.0], [600.0, 400.0]])
    cases = {
        "all_zero": np.zeros((4, 2)),
        "four_equal": np.full((4, 2), 512.0),
        "collinear": np.array([[100.0, 200.0], [200.0, 200.0], [300.0, 200.0], [400.0, 200.0]]),
        "bow_tie": sq[[0, 1, 3, 2]],
        "nan_corner": np.where(np.arange(8).reshape(4, 2) == 5, np.nan, sq),
        # a quad in general position with y of its first corner infinite: the edge determinant stays finite and h33 is
        # infinite, so it passes both early checks and fails only the last one, on the non-finite pose (LATE_FAILURE)
        "inf_corner": np.array([[600.0, np.inf], [705.0, 310.0], [690.0, 415.0], [590.0, 395.0]]),
    }
    return list(cases), np.array(list(cases.values())).astype(np.float32)


def path_sensitive():
    """inputs the solvers do return a pose for, but one that depends on the rounding of the path there: three equal
    corners, a concave quad, corners of the order of 1e30.  For the packing tests only."""
    sq = np.array([[600.0, 300.0], [700.0, 300.0], [700.0, 400.0], [600.0, 400.0]])
    three = sq.copy()
    three[1] = three[2] = three[0]
    concave = sq.copy()
    concave[2] = [620.0, 320.0]
    return np.array([three, concave, sq * 1e30 / 700.0]).astype(np.float32)


# ---- both_minima
MIRROR_SEED, MIRROR_N = 7, 256
MIRROR_BAND = 0.01        # plain and mirrored costs closer than this (relative to the larger) decide nothing
MIRROR_BAND_SHARE = 0.10  # at most this share of the class may lie in the band


def mirror_corners():
    """256 tags tilted 15..50 degrees at z = 300 with 0.3 px of noise, then the 8 frontal tags of half_turns"""
    T = tilted_poses(MIRROR_SEED, MIRROR_N, (15, 50), (300, 300), spread_xy=(0.1, 0.05))
    return np.concatenate([project(T, None, 0.3, MIRROR_SEED + 1000), class_corners("half_turns", "none")[:N_FRONTAL]])


# ---- the packing mix
MIXED_LENSES = ("none", "all5")   # without a lens all six failures fail; through one, collinear and bow_tie round to a pose


def mixed37(lens):
    """37 tags from every class (projected through `lens`), the failures and the path-sensitive inputs among them, interleaved"""
    pools = [failures()[1], path_sensitive()] + [class_corners(n, lens) for n in POSE_CLASSES]
    out, k = [], 0
    while len(out) < 37:
        for p in pools:
            if k < len(p) and len(out) < 37:
                out.append(p[k])
        k += 1
    return np.array(out, dtype=np.float32)


# ---- the comparison of the GPU tests
def pose_error(T, T_ref):
    """per tag: the larger of the largest rotation-entry difference and the translation difference over its length"""
    T, T_ref = np.asarray(T).reshape(-1, 4, 4), np.asarray(T_ref).reshape(-1, 4, 4)
    with np.errstate(all="ignore"):
        eR = np.abs(T[:, :3, :3] - T_ref[:, :3, :3]).reshape(len(T), -1).max(axis=1)
        et = np.sqrt(((T[:, :3, 3] - T_ref[:, :3, 3]) ** 2).sum(axis=1)) / np.sqrt((T_ref[:, :3, 3] ** 2).sum(axis=1))
    e = np.maximum(eR, et)
    return np.where(np.isfinite(e), e, np.inf)


RVEC_NEAR_PI = 1e-3


def rvec_tolerance(rvec_ref, tol):
    """what a rotation known to tol allows its Rodrigues vector: rvec = theta / (2 sin theta) * (differences of two
    entries of R), so an entry error e moves it by about 2 e theta / (2 sin theta) plus the error of theta itself; 4 x
    covers both.  theta / (2 sin theta) is 1/2 at 0 and 1571 at pi - 1e-3."""
    th = np.sqrt((rvec_ref ** 2).sum(axis=-1))
    th = np.clip(th, 1e-8, np.pi - RVEC_NEAR_PI)
    amp = th / (2 * np.sin(th))
    return 4 * np.maximum(amp, 1.0) * tol


def check_poses(got, ref, tol):
    """the GPU tests' comparison of (rvec, tvec, T, ok) with a reference's: a list of complaints, empty if they agree.
    ok must be equal; where ok: T within tol (pose_error), tvec the last column of T, rotation_of(rvec) within 1e-12 of
    T's rotation, and rvec itself within rvec_tolerance wherever the reference's |rvec| < pi - 1e-3 (at pi its sign is
    free); where not ok: rvec, tvec and T all zero."""
    rv, tv, T, ok = got
    rrv, rtv, rT, rok = ref
    bad = []
    if not np.array_equal(np.asarray(ok, bool), np.asarray(rok, bool)):
        return ["ok differs at %s" % np.flatnonzero(np.asarray(ok, bool) != np.asarray(rok, bool)).tolist()]
    for i in range(len(T)):
        if not ok[i]:
            if np.any(rv[i] != 0) or np.any(tv[i] != 0) or np.any(T[i] != 0) or not np.isfinite(T[i]).all():
                bad.append("tag %d: ok = 0 but the record is not zero" % i)
            continue
        e = pose_error(T[i], rT[i])[0]
        if not e <= tol:
            bad.append("tag %d: pose off by %.3g > %.3g" % (i, e, tol))
        if not np.array_equal(T[i, :3, 3], tv[i]) or not np.array_equal(T[i, 3], [0, 0, 0, 1]):
            bad.append("tag %d: T does not carry tvec" % i)
        if not np.abs(PR.rotation_of(rv[i]) - T[i, :3, :3]).max() <= 1e-12:
            bad.append("tag %d: T is not the rotation of rvec" % i)
        if np.sqrt(rrv[i] @ rrv[i]) < np.pi - RVEC_NEAR_PI:
            lim = rvec_tolerance(rrv[i], tol)
            if not np.abs(rv[i] - rrv[i]).max() <= lim:
                bad.append("tag %d: rvec off by %.3g > %.3g" % (i, np.abs(rv[i] - rrv[i]).max(), lim))
    return bad


# ---- references, computed once per session and shared (read-only)
_cache = {}


def _frozen(res):
    for a in res[:4]:
        a.setflags(write=False)
    return res


def statement(name, lens):
    """pnp_ref.solve_pnp(details=True) of class_corners(name, lens), both_minima off"""
    key = ("statement", name, lens)
    if key not in _cache:
        _cache[key] = _frozen(PR.solve_pnp(class_corners(name, lens), K, LENSES[lens], TAG, details=True))
    return _cache[key]


def oracle(name, lens):
    import oracle_lib as O
    key = ("oracle", name, lens)
    if key not in _cache:
        d = LENSES[lens]
        _cache[key] = _frozen(O.solve_pnp(class_corners(name, lens), K, np.zeros(0) if d is None else d, TAG))
    return _cache[key]


def mirror_statement():
    """pnp_ref.solve_pnp(details=True) of mirror_corners() with both_minima on"""
    if "mirror" not in _cache:
        _cache["mirror"] = _frozen(PR.solve_pnp(mirror_corners(), K, None, TAG, both_minima=True, details=True))
    return _cache["mirror"]


def mirror_band(recs):
    """per tag of mirror_statement()'s records: True where the two costs are within MIRROR_BAND of each other"""
    a = np.array([r["cost_plain"] for r in recs])
    b = np.array([r["cost_mirror"] for r in recs])
    with np.errstate(all="ignore"):
        return np.isfinite(b) & (np.abs(a - b) <= MIRROR_BAND * np.maximum(a, b))
