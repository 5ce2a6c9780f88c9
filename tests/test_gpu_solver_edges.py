"""The three device solvers (asl_localize_batch, asl_calibrate_batch, asl_map_batch) against their NumPy statements on
tests/solver_edge_cases.py's edge cases: more than 64 slots per frame up to max_tags 256, ties in the top-8 seed choice,
the gate's limits, 1024 / 1025 / 2100 frames in the one-workgroup kernels, 9, 10, 256 and 1000 map tags (with std).

Integer outputs must match exactly; floats hold the bars of the existing comparisons: 1e-9 relative on poses, K and
distortion, rms within 1e-6, std as test_gpu_calibrate.py / test_gpu_map.py hold it.  Each comparison prints its largest
differences (run with -s to see them)."""
import numpy as np
import pytest

import calib_cases as CC
import calib_ref as CR
import localize_cases as LC
import localize_ref as LR
import map_ref as MR
import solver_edge_cases as E

pytestmark = pytest.mark.gpu

LOC = E.loc_cases()
CAL = E.cal_cases()
MAP = E.map_cases()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0


def same_ints(got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(np.asarray(got[k] != want[k]).ravel())[:8])


def poses_diff(gp, wp):
    used = np.flatnonzero(wp["status"] == 0)
    return max([rel(gp["T"][f], wp["T"][f]) for f in used] or [0.0])


@pytest.mark.parametrize("case", LOC, ids=[c[0] for c in LOC])
def test_localisation_matches_the_statement(gpu_detector, case):
    name, obs, rec, dist, gate, _ = case
    got = gpu_detector.localize(obs, rec, E.K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    want = LR.localize(obs, rec, E.K, dist, LC.TAG_INNER, gate)
    same_ints(got, want, ("status", "n_tags", "n_rejected", "seed_slot"))
    dT = poses_diff(got, want)
    drms = float(np.abs(got["rms_px"] - want["rms_px"]).max())
    dseed = float(np.abs(got["rms_seed_px"] - want["rms_seed_px"]).max())
    print("EDGE localize %-12s T %.2e rms %.2e rms_seed %.2e" % (name, dT, drms, dseed))
    assert dT <= 1e-9
    assert drms <= 1e-6 * max(1.0, want["rms_px"].max()) and dseed <= 1e-6 * max(1.0, want["rms_seed_px"].max())


@pytest.mark.parametrize("case", CAL, ids=[c[0] for c in CAL])
def test_calibration_matches_the_statement(gpu_detector, case):
    name, obs, rec, kw, _ = case
    gr, gp = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    wr, wp = CR.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    same_ints(gr, wr, ("status", "n_frames_used", "n_corners"))
    same_ints(gp, wp, ("status", "n_tags", "n_rejected", "seed_slot"))
    dK = float(np.abs(gr["K"] - wr["K"]).max() / np.abs(wr["K"]).max())
    dd = float(np.abs(gr["dist"] - wr["dist"]).max() / max(1.0, np.abs(wr["dist"]).max()))
    ds = float(np.abs(gr["std"] - wr["std"]).max() / np.abs(wr["std"]).max())
    dT = poses_diff(gp, wp)
    drms = max(abs(float(gr["rms_px"] - wr["rms_px"])), abs(float(gr["rms_init_px"] - wr["rms_init_px"])))
    print("EDGE calibrate %-12s K %.2e dist %.2e std %.2e T %.2e rms %.2e" % (name, dK, dd, ds, dT, drms))
    assert dK <= 1e-9 and dd <= 1e-9 and dT <= 1e-9
    assert np.array_equal(gr["std"] == 0, wr["std"] == 0) and ds <= 1e-7      # a ratio of small sums: a few digits fewer
    assert drms <= 1e-6 * max(1.0, float(wr["rms_init_px"]))


@pytest.mark.parametrize("case", MAP, ids=[c[0] for c in MAP])
def test_map_matches_the_statement(gpu_detector, case):
    name, obs, n_ids, dist, w, kw, _ = case
    gr, gm, gs, gp = gpu_detector.build_map(obs, n_ids, E.K, dist, LC.TAG_INNER, world_id=w, **kw)
    wr, wm, ws, wp = MR.map_frames(obs, n_ids, E.K, dist, LC.TAG_INNER, world_id=w, **kw)[:4]
    same_ints(gr, wr, ("status", "n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "world_id"))
    same_ints(gm, wm, ("valid",))
    same_ints(gp, wp, ("status", "n_tags", "n_rejected", "seed_slot"))
    valid = np.flatnonzero(wm["valid"])
    dG = max(rel(MR.rec4(gm["T"][i]), MR.rec4(wm["T"][i])) for i in valid)
    dT = poses_diff(gp, wp)
    drms = max(abs(float(gr["rms_px"] - wr["rms_px"])), abs(float(gr["rms_seed_px"] - wr["rms_seed_px"])))
    dprms = float(np.abs(gp["rms_px"] - wp["rms_px"]).max())
    free = valid[valid != wr["world_id"]]
    ds = float((np.abs(gs[free] - ws[free]) / ws[free]).max())
    print("EDGE map %-15s tags %.2e cams %.2e rms %.2e cam_rms %.2e std %.2e" % (name, dG, dT, drms, dprms, ds))
    assert dG <= 1e-9 and dT <= 1e-9
    assert drms <= 1e-6 * max(1.0, float(wr["rms_seed_px"])) and dprms <= 1e-6
    np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-12)


def test_the_widest_shapes_give_the_same_bytes_twice(gpu_detector):
    name, obs, rec, dist, gate, _ = [c for c in LOC if c[0] == "wide256_d5"][0]
    a = gpu_detector.localize(obs, rec, E.K, dist, LC.TAG_INNER, max_tag_rms_px=1.0)
    b = gpu_detector.localize(obs, rec, E.K, dist, LC.TAG_INNER, max_tag_rms_px=1.0)
    assert a.tobytes() == b.tobytes()
    name, obs, n_ids, dist, w, kw, _ = [c for c in MAP if c[0] == "tags1000"][0]
    a = gpu_detector.build_map(obs, n_ids, E.K, dist, LC.TAG_INNER, world_id=w, **kw)
    b = gpu_detector.build_map(obs, n_ids, E.K, dist, LC.TAG_INNER, world_id=w, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
