"""The NumPy statement of tag location (tests/locate_ref.py) against the truth of localize_cases' scene, on the CPU."""
import functools

import numpy as np
import pytest

import locate_cases as QC
import locate_ref as QR
import localize_cases as LC
import localize_ref as LR
import pose_cov_ref as PC

POS_TOL, ROT_TOL = 1e-3, 1e-5   # scene units, rad (0.01 mrad): the float32 corners are the floor


@functools.lru_cache(maxsize=None)
def solved(name, sigma_px=None):
    _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
    traces = {}
    out = QR.locate_tags(obs, poses, map_in, QC.K, dist, QC.TAG, gate, min_views, sigma_px=sigma_px, traces=traces)
    return out, traces


def assert_at_truth(map_out, ids):
    tm = QC.truth()
    for i in ids:
        assert map_out["valid"][i] == 1
        dp, dr = QC.pose_errors(map_out["T"][i], tm[i])
        assert dp <= POS_TOL and dr <= ROT_TOL, (i, dp, dr)


def assert_rest_untouched(map_out, map_in, fit):
    rest = fit["status"] != 0
    assert map_out[rest].tobytes() == map_in[rest].tobytes()
    assert np.array_equal(map_out["size"], map_in["size"], equal_nan=True)


@pytest.mark.parametrize("name", ["exact", "mirrored", "dist4", "dist5"])
def test_exact_views_locate_every_odd_tag_at_the_truth(name):
    (map_out, fit), _ = solved(name)
    _, obs, _, map_in, _, _, _ = QC.case(name)
    odd = QC.odd_ids()
    assert (fit["status"][odd] == 0).all() and (fit["n_views"][odd] == len(obs)).all() and (fit["n_rejected"] == 0).all()
    even = [i for i in range(len(map_in)) if i not in odd]
    assert (fit["status"][even] == 1).all() and (fit["seed_frame"][even] == -1).all()
    assert_at_truth(map_out, odd)
    assert_rest_untouched(map_out, map_in, fit)
    assert (fit["rms_px"][odd] < 1e-3).all()


@pytest.mark.parametrize("how", QC.SPOILINGS)
def test_gate_drops_exactly_the_spoiled_view(how):
    (map_out, fit), traces = solved("gate_%s_on" % how)
    for i in QC.odd_ids():
        tv, trace, _, _ = traces[i]
        assert [tv.views[v][0] for v in trace["dropped"]] == [QC.gate_frame(i)], (i, trace["dropped"])
        assert fit["n_rejected"][i] == 1 and fit["n_views"][i] == 7 and fit["status"][i] == 0
    assert_at_truth(map_out, QC.odd_ids())
    (_, fit_off), _ = solved("gate_%s_off" % how)
    assert (fit_off["n_rejected"] == 0).all() and (fit_off["n_views"][QC.odd_ids()] == 8).all()


def test_gate_stops_at_its_cap_and_at_the_last_view():
    (map_out, fit), traces = solved("gate_cap")
    assert fit["status"][1] == 0 and fit["n_rejected"][1] == LR.MAX_GATE_DROPS and fit["n_views"][1] == 17 - LR.MAX_GATE_DROPS
    assert all(traces[1][0].views[v][0] % 2 == 0 for v in traces[1][1]["dropped"])     # only spoiled views went
    assert fit["status"][3] == 0 and fit["n_rejected"][3] == 1 and fit["n_views"][3] == 1


def test_noise_final_cost_is_below_every_candidate():
    (map_out, fit), traces = solved("noise")
    for i in QC.odd_ids():
        tv, trace, (R, t), act = traces[i]
        assert fit["status"][i] == 0 and act.all()
        final = float(tv.costs(R, t, act).sum())
        cands = tv.candidates(act)
        assert len(cands) == 2 * LR.MAX_SEED_SLOTS and all(final <= c for *_, c in cands), i     # the LM only ever accepts a decrease
        assert fit["rms_px"][i] <= fit["rms_seed_px"][i]


@pytest.mark.parametrize("sigma_px", [0.0, 0.5])
def test_covariance_is_the_statement_of_pose_cov_ref(sigma_px):
    (map_out, fit, cov), traces = solved("noise", sigma_px)
    for i in range(len(fit)):
        c = cov[i]
        assert np.array_equal(c["cov"], c["cov"].T)
        if fit["status"][i] != 0:
            assert c["status"] == PC.STATUS_NO_POSE and c["dof"] == 0 and not c["cov"].any() and c["sigma_px"] == sigma_px
            continue
        tv, _, (R, t), act = traces[i]
        cost, H, _ = tv.linearise(R, t, act)
        want, sig, dof, status = PC.cov_from_normal(H, cost, 4 * int(fit["n_views"][i]), R, t, sigma_px, False)
        assert status == PC.STATUS_OK and c["status"] == PC.STATUS_OK
        assert dof == 8 * fit["n_views"][i] - 6 == c["dof"]
        assert np.array_equal(np.tril(c["cov"]), np.tril(want)) and c["sigma_px"] == sig
        assert np.abs(c["cov"] - want).max() <= 1e-12 * np.abs(want).max()
        if sigma_px == 0.0:
            assert abs(sig - np.sqrt(cost / dof)) <= 1e-15 * sig and 0.1 < sig < 1.0     # 0.3 px went in
    # the (r, d) convention: the lower block is the covariance of the tag's position, whose std a 0.3 px noise over 32
    # views puts well below a scene unit
    i = QC.odd_ids()[0]
    assert 0 < np.sqrt(cov["cov"][i][3, 3]) < 0.5


def test_view_count_edges():
    for count, mv, status in ((1, 1, 0), (1, 2, 2), (2, 2, 0), (15, 2, 0), (16, 2, 0), (17, 2, 0)):
        name = "views_edge_%d_min%d" % (count, mv)
        (map_out, fit), _ = solved(name)
        assert fit["status"][1] == status and fit["n_views"][1] == count, name
        if status == 0:
            assert_at_truth(map_out, [1])
        assert_rest_untouched(map_out, QC.case(name)[3], fit)


def test_seed_choice_edges():
    (map_out, fit), traces = solved("seeds_edge")
    tv, trace, _, _ = traces[1]
    assert len(tv.views) == 9 and len(trace["first"]) == 2 * LR.MAX_SEED_SLOTS
    assert 8 not in [v for v, _, _ in trace["first"]]          # the tie in area went to the lower list position
    assert min(tv.area[:8]) == tv.area[8]
    assert fit["status"][1] == 0 and fit["status"][3] == QR.STATUS_NO_PNP and fit["n_views"][3] == 9 and fit["seed_frame"][3] == -1
    tv5, trace5, _, _ = traces[5]
    assert fit["status"][5] == 0 and len({v for v, _, _ in trace5["first"]}) == 1 and fit["seed_frame"][5] != int(np.argmax(tv5.area))
    assert_at_truth(map_out, [1, 5])
    assert map_out["valid"][3] == 0


def test_frame_scan_edges():
    for n, views in ((63, [0, 62]), (64, [0, 63]), (65, [0, 63, 64]), (130, [0, 63, 64, 129])):
        (map_out, fit), traces = solved("frames_edge_%d" % n)
        tv = traces[1][0]
        assert [f for f, _ in tv.views] == views and fit["status"][1] == 0 and fit["n_views"][1] == len(views), n
        assert tv.views[0][1] == 1                              # the id's first slot in frame 0
        assert_at_truth(map_out, [1])


def test_slot_edges():
    (map_out, fit), _ = solved("slots_edge_1")
    assert fit["status"][0] == 0 and fit["n_views"][0] == 4
    tm = QC.truth()
    assert QC.pose_errors(map_out["T"][0], tm[0])[0] <= POS_TOL
    (map_out, fit), _ = solved("slots_edge_256")
    map_in = QC.case("slots_edge_256")[3]
    located = np.flatnonzero(fit["status"] == 0)
    assert list(located) == [5, 1000, 2114]
    for new, old in ((5, 5), (1000, 3), (2114, 1)):
        dp, dr = QC.pose_errors(map_out["T"][new], tm[old])
        assert dp <= POS_TOL and dr <= ROT_TOL
    assert fit["status"][77] == QR.STATUS_FEW_VIEWS and fit["n_views"][77] == 0 and fit["status"][9] == 1 and (fit["status"][20:40] == 1).all()
    assert_rest_untouched(map_out, map_in, fit)


def test_wanted_ids_and_a_tag_of_its_own_size():
    (map_out, fit), _ = solved("wanted")
    map_in = QC.case("wanted")[3]
    assert fit["status"][1] == 1 and fit["status"][3] == 1 and fit["status"][0] == 1
    odd = [i for i in QC.odd_ids() if i not in (1, 3)]
    assert (fit["status"][odd] == 0).all()
    assert_at_truth(map_out, odd)
    assert map_out["size"][QC.SIZED_ID] == np.float32(QC.SIZED_SIDE)
    assert_rest_untouched(map_out, map_in, fit)


def test_an_extended_map_localises_frames_that_see_only_new_tags():
    (map_out, fit), _ = solved("exact")
    cams = LC.trajectory(16)[8:12]
    obs = QC.block(cams)
    even = (obs["id"] % 2 == 0)
    obs["id"][even] = -1
    obs["flags"][even] = 0
    got = LR.localize(obs, map_out, QC.K, None, QC.TAG)
    assert (got["status"] == 0).all() and (got["n_tags"] >= 5).all()
    for g, (p, r) in zip(got, cams):
        t = LC.world_from_camera(p, r)
        assert np.linalg.norm(g["T"][:3, 3] - t[:3, 3]) <= POS_TOL and LC.rot_err(g["T"], t) <= ROT_TOL
