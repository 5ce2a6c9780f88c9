"""The NumPy statements of the three pose solvers (localize_ref, calib_ref, map_ref) on tests/solver_edge_cases.py's edge
cases: each must recover the truth, make the seed choice the case was built for and drop what the gate must drop, so that
the device comparison (tests/test_gpu_solver_edges.py) has a reference known to be right at these shapes.  No GPU needed.

Poses are held to the truth as far as float32 corners allow: the localisation and calibration to 1e-6 relative, the map
(whose tags are also unknowns, several seen in one view only) to 1e-5 of the scene's extent."""
import numpy as np
import pytest

import calib_cases as CC
import calib_ref as CR
import localize_cases as LC
import localize_ref as LR
import map_cases as MC
import map_ref as MR
import solver_edge_cases as E

LOC = E.loc_cases()
CAL = E.cal_cases()
MAP = E.map_cases()


@pytest.mark.parametrize("case", LOC, ids=[c[0] for c in LOC])
def test_localisation_statement(case):
    name, obs, rec, dist, gate, ex = case
    traces = []
    out = LR.localize(obs, rec, E.K, dist, LC.TAG_INNER, gate, traces=traces)
    assert (out["status"] == 0).all()
    if name.startswith("wide"):
        assert all((o["flags"] & 1).sum() > 64 for o in obs)
    for f, T in enumerate(ex.get("truth", [])):
        assert LC.rel_err(out["T"][f], T) <= 1e-6, (f, LC.rel_err(out["T"][f], T))
    if "n_tags" in ex:
        assert out["n_tags"].tolist() == ex["n_tags"]
    if "n_rejected" in ex:
        assert out["n_rejected"].tolist() == ex["n_rejected"]
    for f, want in ex.get("top_k", {}).items():
        assert traces[f]["top_k"] == want, (f, traces[f]["top_k"], want)
        assert int(out["seed_slot"][f]) == ex["seed_slot"][f]
    for f, want in ex.get("dropped", {}).items():
        assert traces[f]["dropped"] == want
    for f, want in ex.get("dropped_prefix", {}).items():
        assert traces[f]["dropped"][:len(want)] == want, traces[f]["dropped"]
        r = traces[f]["gate_rms"][0]                    # every slot takes part: gate_rms is indexed by slot
        assert (obs[f]["flags"] & 1).all() and r[want[0]] == r[want[1]] == r.max()   # the tie is at the top, bit for bit
    if "dropped_from" in ex:
        for f, tr in enumerate(traces):
            assert len(tr["dropped"]) == 8 and {int(obs[f]["id"][s]) for s in tr["dropped"]} <= set(ex["dropped_from"])
    if ex.get("all_over"):
        assert (traces[0]["gate_rms"][0] > gate).all() and traces[0]["dropped"] == [2, 1]


def test_tie_rule_is_the_lower_position():
    """localize_ref.top_k on the tie layouts the kernels see: equal areas 64 apart, the boundary inside the tie"""
    mixed = [0.0] * 200
    for s in (5, 69, 133, 197, 6, 70, 134, 198, 7):
        mixed[s] = 3.0
    mixed[100], mixed[101] = 4.0, 2.0
    assert LR.top_k(mixed) == [5, 6, 7, 69, 70, 100, 133, 134]
    tied = [0.0] * 200
    for s in (5, 69, 133, 197, 6, 70, 134, 198, 7):
        tied[s] = 3.0
    assert LR.top_k(tied) == [5, 6, 7, 69, 70, 133, 134, 197]


@pytest.mark.parametrize("case", CAL, ids=[c[0] for c in CAL])
def test_calibration_statement(case):
    name, obs, rec, kw, ex = case
    res, poses = CR.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    assert res["status"] == 0 and res["n_frames_used"] == len(ex["truth"])
    assert np.abs(res["K"] - CC.K_TRUE).max() <= 1e-6 * CC.K_TRUE[0, 0]
    # the lens over the whole image, also where no tag is seen (max_tags 65 keeps the top rows of the grid only)
    assert CC.field_err(res["K"], res["dist"][:kw["n_dist"]], CC.K_TRUE, ex["dist"]) <= 1e-2
    for f, T in ex["truth"].items():
        assert poses["status"][f] == 0 and LC.rel_err(poses["T"][f], T) <= 1e-6, (f, LC.rel_err(poses["T"][f], T))
    assert (poses["status"][[f for f in range(len(obs)) if f not in ex["truth"]]] == 1).all()
    if "n_tags" in ex:
        assert (poses["n_tags"][list(ex["truth"])] > 64).all() and poses["n_tags"].max() == ex["n_tags"]
    if "n_tags0" in ex:
        assert poses["n_tags"][0] == ex["n_tags0"]


@pytest.mark.parametrize("case", MAP, ids=[c[0] for c in MAP])
def test_map_statement(case):
    name, obs, n_ids, dist, w, kw, ex = case
    res, tmap, std, poses = MR.map_frames(obs, n_ids, E.K, dist, LC.TAG_INNER, world_id=w, **kw)[:4]
    assert res["status"] == 0 and res["n_obs_dropped"] == 0
    if "n_tags" in ex:
        assert res["n_tags"] == ex["n_tags"]
    valid = np.flatnonzero(tmap["valid"])
    assert (std[valid[valid != res["world_id"]]] > 0).all()
    if "scene" in ex:
        tags, cams = ex["scene"]
        used = [f for f in range(len(obs)) if cams[f] is not None] if len(cams) == len(obs) else list(range(len(obs)))
        assert (poses["status"][used] == 0).all() and res["n_frames_used"] == len(used)
        et, er, ec = MC.map_errors(tmap, poses[used], tags, [cams[f] for f in used] if len(cams) == len(obs) else cams,
                                   int(res["world_id"]))
        extent = np.ptp([t["position"] for t in tags], axis=0).max()
        assert max(et, ec) <= 1e-5 * extent and er <= 1e-4, (et, ec, er, extent)
    if name == "repeat_id":
        assert poses["n_tags"][2] == (obs["id"][2] >= 0).sum() - 1
