"""The NumPy statement of rig tag location (tests/locate_rig_ref.py) on the CPU: with one camera at the identity it is
locate_ref.py, it recovers tags that only a camera without a mapped tag sees and tags two cameras see at once, and the view
lists of tests/locate_rig_cases.py have the counts and the order the cases are built for.  No GPU."""
import functools

import numpy as np
import pytest

import localize_cases as LC
import locate_cases as QC
import locate_ref as QR
import locate_rig_cases as ZC
import locate_rig_ref as ZR

# world<-tag against the truth on ZC.RECOVER (true PnP poses, corners rounded to float32): 4 x the worst measured value,
# rounded up to one digit.  Measured: rear_only 2.54e-4 units, 6.32e-6 rad (6 views of a 72 px tag in the rear camera);
# mixed_models 9.38e-5 units, 4.39e-6 rad; both_cameras and sized 4.48e-5 units, 2.43e-6 rad.
TRUTH_UNITS, TRUTH_RAD = 2e-3, 3e-5
ONE_CAMERA = ("exact", "wanted", "gate_cap", "frames_edge_130", "dist5")


@functools.lru_cache(maxsize=None)
def statement(name):
    c = ZC.case(name)
    traces = {}
    out = ZR.locate_tags_rig(c["obs"], c["poses"], c["map_in"], c["rig"], ZC.TAG, c["gate"], c["min_views"], sigma_px=0.0, traces=traces)
    return out, traces


@pytest.mark.parametrize("name", ONE_CAMERA)
def test_one_camera_at_the_identity_is_the_single_camera_statement(name):
    _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
    wm, wf, wc = QR.locate_tags(obs, poses, map_in, QC.K, dist, QC.TAG, gate, min_views, sigma_px=0.0)
    gm, gf, gc = ZR.locate_tags_rig(obs[None], poses, map_in, ZC.solo(QC.K, dist), QC.TAG, gate, min_views, sigma_px=0.0)
    for k in ("status", "n_views", "n_rejected", "seed_frame", "seed_mirrored", "reserved"):
        assert np.array_equal(gf[k], wf[k]), (name, k)
    assert np.array_equal(gm["valid"], wm["valid"]) and gm["size"].tobytes() == wm["size"].tobytes()
    assert np.array_equal(gc["status"], wc["status"]) and np.array_equal(gc["dof"], wc["dof"])
    assert (wf["status"] == 0).any()
    for i in np.flatnonzero(wf["status"] == 0):
        assert LC.rel_err(gm["T"][i], wm["T"][i]) <= 1e-12, (name, i)
        assert abs(gf["rms_px"][i] - wf["rms_px"][i]) <= 1e-12 * max(1.0, wf["rms_px"][i])
        assert np.abs(gc["cov"][i] - wc["cov"][i]).max() <= 1e-9 * np.abs(wc["cov"][i]).max()
    rest = wf["status"] != 0
    assert gm[rest].tobytes() == wm[rest].tobytes()


@pytest.mark.parametrize("name", ZC.RECOVER)
def test_the_truth_is_recovered(name):
    c = ZC.case(name)
    (m, fit, cov), _ = statement(name)
    assert c["truth"]
    for i, T in c["truth"].items():
        assert fit["status"][i] == 0 and fit["n_rejected"][i] == 0 and m["valid"][i] == 1, (name, i)
        dp, dr = QC.pose_errors(m["T"][i], T)
        print("%s id %d: %d views, %.3g units and %.3g rad from the truth" % (name, i, fit["n_views"][i], dp, dr))
        assert dp <= TRUTH_UNITS and dr <= TRUTH_RAD, (name, i, dp, dr)
        assert cov["status"][i] == 0 and cov["dof"][i] == 8 * fit["n_views"][i] - 6
    kept = c["map_in"]["valid"] == 1
    assert m[kept].tobytes() == c["map_in"][kept].tobytes()                  # the entries the map had: byte for byte


def test_a_camera_that_sees_no_mapped_tag_locates_its_tags():
    c = ZC.case("rear_only")
    (m, fit, _), traces = statement("rear_only")
    for i in (2, 3):
        assert [cam for _, cam, _ in traces[i][0].views] == [1] * 6 and fit["n_views"][i] == 6
    # camera 1 alone has no pose to be located from: the single-camera call on its records finds every frame without one
    from localize_ref import localize
    alone = localize(c["obs"][1], c["map_in"], c["rig"].cameras[1].K, None, ZC.TAG)
    assert (alone["status"] != 0).all()
    _, f1 = QR.locate_tags(c["obs"][1], alone, c["map_in"], c["rig"].cameras[1].K, None, ZC.TAG)
    assert (f1["status"][2:4] == QR.STATUS_FEW_VIEWS).all()


def test_the_sized_tag_is_solved_at_its_own_side():
    c = ZC.case("sized")
    (m, fit, _), traces = statement("sized")
    tv = traces[ZC.SIZED_ID][0]
    assert tv.own and tv.h != traces[1][0].h and {cam for _, cam, _ in tv.views} == {0, 1}
    assert m["size"][ZC.SIZED_ID] == ZC.SIZED_SIDE
    unsized = c["map_in"].copy()
    unsized["size"][ZC.SIZED_ID] = 0.0
    m0, f0 = ZR.locate_tags_rig(c["obs"], c["poses"], unsized, c["rig"], ZC.TAG)
    assert f0["rms_px"][ZC.SIZED_ID] > 1.0 > fit["rms_px"][ZC.SIZED_ID]      # at the call's size the views of the two cameras disagree


@pytest.mark.parametrize("name", [n for n in ZC.CASES if n.startswith(("both_cameras", "mixed_models", "frames_edge", "views_edge", "gate_cap"))])
def test_the_view_lists_have_the_counts_and_the_order_the_cases_are_built_for(name):
    c = ZC.case(name)
    (_, fit, _), traces = statement(name)
    for i, views in c["views"].items():
        got = [(f, cam) for f, cam, _ in traces[i][0].views]
        assert got == views and got == sorted(got), (name, i, got)
        assert fit["n_views"][i] + fit["n_rejected"][i] == len(views)
    if name.startswith("frames_edge"):
        per_frame = np.bincount([f for f, _ in c["views"][1]], minlength=c["obs"].shape[1])
        assert set(per_frame) == {0, 1, 2}                                   # the lanes' counts across the chunk edges
    if name == "views_edge_2":
        assert c["min_views"] == 2 and fit["status"][1] == 0 and c["views"][1] == [(0, 0), (0, 1)]


def test_the_frames_that_must_not_count_do_not_count():
    c = ZC.case("frames_edge_130")
    (m, fit, _), traces = statement("frames_edge_130")
    tv = traces[1][0]
    assert not {10, 11, 12, 13} & {f for f, _, _ in tv.views} and (64, 0, QC.slot_of(c["obs"][0], 64, 1)) in tv.views
    assert tv.views[0] == (0, 0, QC.slot_of(c["obs"][0], 0, 1)) and tv.views[0][2] != 3      # the first slot, not the spoiled second
    assert fit["status"][1] == 0 and fit["n_views"][1] == 6 and fit["rms_px"][1] < 1e-3      # a spoiled view would show
    dp, dr = QC.pose_errors(m["T"][1], c["truth"][1])
    assert dp <= TRUTH_UNITS and dr <= TRUTH_RAD


def test_the_top_8_leave_out_the_later_of_two_equal_areas_across_cameras():
    c = ZC.case("mixed_models")
    _, traces = statement("mixed_models")
    i = ZC.TOP8_ID
    tv, trace = traces[i][0], traces[i][1]
    seeding = [v for v in range(len(tv.views)) if tv.flags[v] & 2]
    assert len(seeding) == 9 and {tv.views[v][1] for v in seeding} == {0, 1}
    used = sorted({v for v, _, _ in trace["first"]})
    assert used == [v for v in seeding if v != c["left_out"][i]] and c["left_out"][i] == max(seeding)
    # areas are pixels as they are: every view of the long-focus camera is larger than the two of the other
    a = np.array(tv.area)
    assert a[[v for v in seeding if tv.views[v][1] == 0]].min() > a[[v for v in seeding if tv.views[v][1] == 1]].max()


@pytest.mark.parametrize("how", QC.SPOILINGS)
def test_the_gate_drops_one_cameras_view_and_keeps_the_other_of_the_frame(how):
    c = ZC.case("gate_per_view_%s_on" % how)
    (m, fit, _), traces = statement(c["name"])
    (_, off, _), _ = statement("gate_per_view_%s_off" % how)
    for i, (f, cam) in c["spoiled"].items():
        tv, trace, _, act = traces[i]
        pos = [(v[0], v[1]) for v in tv.views]
        assert fit["n_rejected"][i] == 1 and trace["dropped"] == [pos.index((f, cam))], (how, i)
        assert act[pos.index((f, 0))] and fit["rms_px"][i] < 1e-3 < off["rms_px"][i]
        assert off["n_rejected"][i] == 0
        dp, dr = QC.pose_errors(m["T"][i], c["truth"][i])
        assert dp <= TRUTH_UNITS and dr <= TRUTH_RAD, (how, i, dp, dr)


def test_the_gate_stops_at_its_cap_and_never_drops_the_last_view():
    (_, fit, _), traces = statement("gate_cap")
    assert fit["n_rejected"][1] == 8 and fit["n_views"][1] == 9
    assert fit["n_rejected"][3] == 1 and fit["n_views"][3] == 1 and len(traces[3][1]["dropped"]) == 1  # two views cannot tell which is spoiled


def test_noise_ends_no_tag_mirrored():
    c = ZC.case("noise")
    (m, fit, _), _ = statement("noise")
    for i, T in c["truth"].items():
        # 0.3 px a coordinate is 0.42 px a corner; over the >= 48 - 6 degrees of freedom of 6 views the RMS scatters by
        # 1 / sqrt(2 x 42) = 11 % of that, and 4 such deviations either way are 0.24 .. 0.61 px
        assert fit["status"][i] == 0 and 0.24 < fit["rms_px"][i] < 0.61, (i, fit["rms_px"][i])
        assert QC.pose_errors(m["T"][i], T)[1] < 0.5, i                       # a mirrored minimum is about 1 rad off
