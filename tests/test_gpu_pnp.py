"""The per-tag PnP kernels (k_pnp_batch behind asl_solve_pnp_batch, k_pnp_dets behind the detect calls with a camera;
aprilslam_amd/csrc/k_pnp.inc) at their wave-packing, pose, lens and failure edges, against the NumPy statement
(pnp_ref.py) and the C oracle on the cases of pnp_cases.py.  The tolerances are pnp_cases.tolerance(): 10 x the spread
between the two references, which test_pnp_ref.py measures on the CPU; none of them comes from the device's output.

ASL_PNP_TPW is the tags-per-wave override pnp_tpw() (aprilslam.hip) reads on every call: unset, a launch below 2048 tags
runs 1 tag a wave beside 15 dummy quads, and only from 2048 / 4096 / 8192 / 16384 tags on 2 / 4 / 8 / 16.

What no case here reaches:
  - the clamp of the detection count to max_dets in k_pnp_dets (a frame with more detections than the detector's list
    holds), and its batch_poisoned() exit;
  - an ok = 0 record written by k_pnp_dets: the detector returns no quad whose four corners have no pose, so the zeros of
    a failed DetRec are the same two stores as k_pnp_batch's, checked there only;
  - chol6_solve_tri_dev refusing a finite system (a damped normal matrix that is not positive definite), the 12th try of a
    linearisation and the 20th linearisation: no case is known to need them, and none is asserted to;
  - the mirrored solve of both_minima under a lens (the mirror class has none), and rodrigues_dev below 2.2e-16 other
    than through rvec = 0.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O  # noqa: F401  (pnp_cases.oracle builds it on first use)
import pnp_cases as PC
import pnp_ref as PR
import tag_sheet as TS
from aprilslam_amd import _lib, synth

pytestmark = pytest.mark.gpu
TPW = "ASL_PNP_TPW"
PACKINGS = (None, 1, 2, 3, 5, 8, 16)


@pytest.fixture(scope="module")
def det():
    d = _lib.Detector("tagStandard41h12", decimate=1.0, id_limit=0)
    yield d
    d.close()


def set_tpw(monkeypatch, tpw):
    if tpw is None:
        monkeypatch.delenv(TPW, raising=False)
    else:
        monkeypatch.setenv(TPW, str(tpw))


def solve(det, corners, lens, both_minima=False):
    det.set_pnp_both_minima(both_minima)
    try:
        return det.solve_pnp(corners, PC.K, PC.LENSES[lens], PC.TAG)
    finally:
        det.set_pnp_both_minima(False)


def same_bytes(a, b):
    """per tag: whether rvec, tvec, T and ok of the two results are the same bytes"""
    return [all(x[i].tobytes() == y[i].tobytes() for x, y in zip(a, b)) for i in range(len(a[3]))]


def take(res, idx):
    return tuple(a[idx] for a in res)


def alone(det, corners, lens, on):
    """every tag in a launch of its own (1 tag a wave, 15 dummy quads)"""
    parts = [solve(det, corners[i:i + 1], lens, on) for i in range(len(corners))]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


# ---- 1. packing changes no bit
@pytest.mark.parametrize("on", [False, True], ids=["plain", "both_minima"])
@pytest.mark.parametrize("lens", PC.MIXED_LENSES)
def test_packing_changes_no_bit(det, monkeypatch, lens, on):
    c = PC.mixed37(lens)
    set_tpw(monkeypatch, None)
    ref = alone(det, c, lens, on)
    assert 4 <= (~ref[3]).sum() <= 9 and ref[3].sum() >= 28   # failures and live tags side by side
    rev = np.arange(len(c))[::-1]
    for tpw in PACKINGS:
        set_tpw(monkeypatch, tpw)
        for idx in [np.arange(len(c)), rev] + [np.arange(n) for n in (1, 15, 16, 17)]:
            same = same_bytes(solve(det, c[idx], lens, on), take(ref, idx))
            assert all(same), (tpw, len(idx), [int(idx[i]) for i, s in enumerate(same) if not s])


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4096, 32768])
def test_tiled_launches_across_the_packing_thresholds(det, monkeypatch, n):
    """pnp_tpw itself: 1 tag a wave at 2047, 2 at 2048 and 2049 (an odd count: a half-filled last wave), 4 at 4096, 16 at 32768"""
    set_tpw(monkeypatch, None)
    c = PC.mixed37("all5")
    idx = np.arange(n) % len(c)
    for on in (False, True):
        ref = alone(det, c, "all5", on)
        got = solve(det, c[idx], "all5", on)
        for g, r in zip(got, ref):
            assert g.tobytes() == r[idx].tobytes(), (n, on, np.flatnonzero((g != r[idx]).reshape(n, -1).any(axis=1))[:8])


def test_no_tags_is_ok_and_writes_nothing(det):
    keep, Kp, dpp, nd = _lib._camera(PC.K, PC.LENSES["all5"])
    c = np.zeros((1, 4, 2), np.float32)
    rv, tv, T, ok = np.full(3, 7.5), np.full(3, 7.5), np.full(16, 7.5), np.full(1, 9, np.uint8)
    dp = C.POINTER(C.c_double)
    rc = det._L.asl_solve_pnp_batch(det._h, c.ctypes.data_as(C.POINTER(C.c_float)), Kp, dpp, nd, PC.TAG, rv.ctypes.data_as(dp),
                                    tv.ctypes.data_as(dp), T.ctypes.data_as(dp), ok.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    assert rc == 0 and (rv == 7.5).all() and (tv == 7.5).all() and (T == 7.5).all() and ok[0] == 9
    rv, tv, T, ok = det.solve_pnp(np.zeros((0, 4, 2), np.float32), PC.K, None, PC.TAG)
    assert rv.shape == (0, 3) and tv.shape == (0, 3) and T.shape == (0, 4, 4) and ok.shape == (0,)


# ---- 2. failed records
@pytest.mark.parametrize("tpw", [None, 16])
def test_failed_records_are_zero(det, monkeypatch, tpw):
    """ok = 0 and zeros in rvec, tvec and T for the six inputs without a pose -- the early exits of pnp_quad_dev (degenerate
    quads, the NaN corner) and the late one (the infinite corner: non-finite after the solve) --, alone and between live tags."""
    names, bad = PC.failures()
    live = PC.class_corners("tilts", "none")[:10]
    mix = np.concatenate([live[:3], bad[:2], live[3:5], bad[2:5], live[5:], bad[5:]])
    where = np.r_[3, 4, 7, 8, 9, 15]
    set_tpw(monkeypatch, None)
    ref_live = alone(det, live, "none", False)
    set_tpw(monkeypatch, tpw)
    for on in (False, True):
        rv, tv, T, ok = solve(det, bad, "none", on)
        for i, name in enumerate(names):
            assert not ok[i], name
            assert not rv[i].any() and not tv[i].any() and not T[i].any() and np.isfinite(T[i]).all(), (name, rv[i], tv[i], T[i])
    got = solve(det, mix, "none")
    assert np.array_equal(np.flatnonzero(~got[3]), where)
    assert not got[0][where].any() and not got[1][where].any() and not got[2][where].any()
    keep = np.setdiff1d(np.arange(len(mix)), where)
    assert all(same_bytes(take(got, keep), ref_live))
    assert PC.check_poses(got, PR.solve_pnp(mix, PC.K, None, PC.TAG), PC.tolerance("tilts")) == []


# ---- 3. poses against both references at full waves
@pytest.mark.parametrize("lens", list(PC.LENSES))
def test_poses_against_the_statement_and_the_oracle(det, monkeypatch, lens):
    names = [n for n, l in PC.pose_classes() if l == lens]
    parts = [PC.class_corners(n, lens) for n in names]
    if lens == "none":   # without a lens the six failures fail in the oracle too: ok has to follow it
        names.append("failures")
        parts.append(PC.failures()[1])
    set_tpw(monkeypatch, 16)
    got = solve(det, np.concatenate(parts), lens)
    assert len(got[3]) >= 100   # full waves
    start, complaints = 0, []
    for name, part in zip(names, parts):
        g = take(got, slice(start, start + len(part)))
        start += len(part)
        if name == "failures":
            st = PR.solve_pnp(part, PC.K, None, PC.TAG)
            orc = O.solve_pnp(part, PC.K, np.zeros(0), PC.TAG)
            orc = (np.zeros_like(orc[0]), np.zeros_like(orc[1]), np.zeros_like(orc[2]), orc[3])   # the oracle's ok; its buffers are not written
            tol = 0.0
        else:
            st, orc, tol = PC.statement(name, lens)[:4], PC.oracle(name, lens), PC.tolerance(name)
            print("%s / %s: off the statement by %.3g, off the oracle by %.3g, tolerance %.3g"
                  % (name, lens, PC.pose_error(g[2], st[2]).max(), PC.pose_error(g[2], orc[2]).max(), tol))
        complaints += ["%s / %s vs statement: %s" % (name, lens, b) for b in PC.check_poses(g, st, tol)]
        complaints += ["%s / %s vs oracle: %s" % (name, lens, b) for b in PC.check_poses(g, orc, tol)]
        if name == "half_turns":
            assert np.array_equal(g[0][3 * PC.N_FRONTAL], np.zeros(3)) and np.array_equal(g[2][3 * PC.N_FRONTAL, :3, :3], np.eye(3))
    assert not complaints, "\n".join(complaints)


# ---- 4. both_minima
def test_both_minima_against_the_statement(det, monkeypatch):
    c = PC.mirror_corners()
    n = PC.MIRROR_N
    rv, tv, T, ok, recs = PC.mirror_statement()
    cam = PR.camera(PC.K, None)
    set_tpw(monkeypatch, 16)
    off, on = solve(det, c, "none", False), solve(det, c, "none", True)
    set_tpw(monkeypatch, None)
    assert all(same_bytes(solve(det, c, "none", True), on))
    assert off[3].all() and on[3].all()
    assert all(same_bytes(take(on, slice(n, None)), take(off, slice(n, None))))   # frontal: no second pose, the same bytes
    cost_off = np.array([PR.cost(off[2][i], c[i], cam) for i in range(n)])
    cost_on = np.array([PR.cost(on[2][i], c[i], cam) for i in range(n)])
    assert (cost_on <= cost_off).all(), np.flatnonzero(cost_on > cost_off)
    band = PC.mirror_band(recs)[:n]
    assert band.sum() <= PC.MIRROR_BAND_SHARE * n
    err = PC.pose_error(on[2][:n], T[:n])
    moved = np.array([not np.array_equal(on[2][i], off[2][i]) for i in range(n)])
    print("both_minima: %d of %d moved to the mirrored minimum (statement: %d), %d left out; worst distance to the statement's choice %.3g"
          % (moved.sum(), n, sum(r["mirrored"] for r in recs[:n]), band.sum(), err[~band].max()))
    assert (err[~band] <= PC.tolerance("noisy")).all(), (np.flatnonzero(~band & (err > PC.tolerance("noisy"))), err[~band].max())
    assert np.array_equal(moved[~band], np.array([r["mirrored"] for r in recs[:n]])[~band])


# ---- 5. the fused path, packed
def test_fused_path_equals_the_batch_kernel_at_every_packing(det, family, monkeypatch):
    """k_pnp_dets against k_pnp_batch: one tag sheet's poses from detect_host(K=...), 16 and 5 tags a wave and as pnp_tpw
    decides, against solve_pnp of the detections' float32 corners"""
    img = TS.tag_sheet(family, 640, 480, 4, 12, n=53)
    K, dist = synth.camera_matrix(640, 480), PC.LENSES["all5"]
    runs = {}
    for tpw in (16, 5, None):
        set_tpw(monkeypatch, tpw)
        dets, poses, npf = det.detect_host(img, channels=1, K=K, dist=dist, tag_size=PC.TAG)
        assert len(dets) == len(poses) == 53 and len(dets) > 32 and len(dets) % 16 != 0 and poses["ok"].all()
        rv, tv, T, ok = det.solve_pnp(dets["corners"].astype(np.float32), K, dist, PC.TAG)
        assert ok.all()
        assert poses["rvec"].tobytes() == rv.tobytes() and poses["tvec"].tobytes() == tv.tobytes() and poses["T"].tobytes() == T.tobytes()
        runs[tpw] = (dets.tobytes(), poses.tobytes())
    assert runs[16] == runs[None] and runs[5] == runs[None]
