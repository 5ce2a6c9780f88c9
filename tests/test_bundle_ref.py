"""The NumPy statement of the tag-bundle calls (tests/bundle_ref.py) on the inputs of tests/bundle_cases.py, and the host
side of aprilslam_amd/bundles.py.  No GPU.

The relative covariance's device bar is derived here: e is the largest difference, over every posed pair of the cases and
both references, between the float64 and the np.longdouble evaluation of C_ab, per element over sqrt(C_ii C_jj).  The
device evaluates the same sum in another order of float64 operations, so it is held to max(10 e, 1e-12)
(bundle_cases.device_cov_bar, used by tests/test_gpu_bundles.py).  Measured: e = 1.7e-14 (x86-64, 80-bit long double), so the bar is 1e-12."""
import numpy as np
import pytest

import bundle_cases as BC
import bundle_ref as BR
import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import _lib
from aprilslam_amd.bundles import BundleResult, BundleSet
from aprilslam_amd.localize import TagMap


def _random_pose(rng, scale):
    T = np.eye(4)
    T[:3, :3] = LR.rodrigues(rng.normal(size=3))
    T[:3, 3] = rng.normal(size=3) * scale
    return T


def test_jacobians_against_central_differences():
    """J_a and J_b of the statement against central differences of the exact composition T_a inv(T_b) under the (r, d)
    perturbations of asl_pose_cov.  Step h = 1e-5: the truncation error is O(h^2) of the second derivatives (entries up to
    |p| ~ 100), the rounding error O(eps |p| / h) ~ 1e-9; the bar is 1e-6 of the largest entry of the Jacobian."""
    rng = np.random.default_rng(5)
    h = 1e-5
    for trial in range(6):
        Ta, Tb = _random_pose(rng, 100.0), _random_pose(rng, 60.0)
        _, Ja, Jb = BR.jacobians(Ta, Tb)
        Na, Nb = np.zeros((6, 6)), np.zeros((6, 6))
        z = np.zeros(6)
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Na[:, k] = (BR.compose_exact(Ta, d, Tb, z) - BR.compose_exact(Ta, -d, Tb, z)) / (2 * h)
            Nb[:, k] = (BR.compose_exact(Ta, z, Tb, d) - BR.compose_exact(Ta, z, Tb, -d)) / (2 * h)
        ea, eb = np.abs(Ja - Na).max() / np.abs(Ja).max(), np.abs(Jb - Nb).max() / np.abs(Jb).max()
        print("trial %d: J_a off by %.2e, J_b by %.2e of their largest entries" % (trial, ea, eb))
        assert ea <= 1e-6 and eb <= 1e-6


def test_relative_of_a_pose_to_itself():
    """relative(a, a): the identity; with the same covariance on both sides the rotation block cancels to nothing but its
    own (r_ab = r_a - r_b of two independent errors: 2 C_rr), and the record of b == ref is the identity with zeros"""
    rng = np.random.default_rng(6)
    T = _random_pose(rng, 50.0)
    A = rng.normal(size=(6, 6))
    C = A @ A.T * 1e-4
    Tab, Cab = BR.relative(T, C, T, C)
    assert np.abs(Tab - np.eye(4)).max() <= 1e-13
    assert np.abs(Cab[:3, :3] - 2 * C[:3, :3]).max() <= 1e-12 * np.abs(C).max()
    assert np.abs(Cab - Cab.T).max() <= 1e-15 * np.abs(Cab).max()
    _, p, c = BC.statement("camera", 16)
    for ref in (0, 2):
        rel = BR.relative_records(p, c, ref)
        assert (rel["T"][:, ref] == np.eye(4)).all() and not rel["cov"][:, ref].any()
        assert rel["status"][:, ref].tolist() == [int(s != 0) for s in p["status"][:, ref]]


def test_status_table():
    _, p, c = BC.statement("camera", 16)
    assert p["status"].tolist() == BC.expected_status().tolist()
    rel = BR.relative_records(p, c, 0)
    # reference 0 has no pose in frame 3: the whole frame is 1; bundle 1 has none in frame 1
    assert rel["status"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 1], [0, 0, 0]]
    for f, b in ((1, 1), (3, 0), (3, 1), (3, 2)):
        assert (rel["T"][f, b] == np.eye(4)).all() and not rel["cov"][f, b].any()
    # status 2: no covariances at all, or one of the two with a status of its own
    none = BR.relative_records(p, None, 2)
    assert none["status"].tolist() == [[2, 2, 0], [2, 1, 0], [2, 2, 0], [1, 2, 0], [2, 2, 0]]
    full = BR.relative_records(p, c, 2)
    assert not none["cov"].any() and np.array_equal(none["T"], full["T"])
    bad = c.copy()
    bad["status"][4, 1] = 2
    bad["cov"][4, 1] = 0
    one = BR.relative_records(p, bad, 2)
    assert one["status"][4].tolist() == [0, 2, 0] and not one["cov"][4, 1].any() and np.array_equal(one["T"][4, 1], full["T"][4, 1])
    assert one[:4].tobytes() == full[:4].tobytes()


@pytest.mark.parametrize("kind,max_tags", [("camera", mt) for mt in BC.MAX_TAGS] + [("rig", 4)])
def test_statement_recovers_the_truth_on_exact_corners(kind, max_tags):
    """every (frame, bundle) meant to be posed has status 0, and bundle<-camera and ref<-bundle are the true ones to 1e-6
    relative (localize_cases.rel_err; the corners are exact but for their rounding to float32)"""
    _, p, c = BC.statement(kind, max_tags)
    truth = BC.truth(kind == "rig")
    assert p["status"].tolist() == BC.expected_status().tolist()
    assert ((p["status"] == 0) == BC.meant_posed()).all() and (c["status"][BC.meant_posed()] == 0).all()
    worst = 0.0
    for f, b in zip(*np.nonzero(BC.meant_posed())):
        worst = max(worst, LC.rel_err(p["T"][f, b], truth[f, b]))
    for ref in (0, 2):
        rel = BR.relative_records(p, c, ref)
        for f, b in zip(*np.nonzero(rel["status"] == 0)):
            worst = max(worst, LC.rel_err(rel["T"][f, b], truth[f, ref] @ np.linalg.inv(truth[f, b])))
    print(kind, max_tags, "worst pose error against the truth %.2e" % worst)
    assert worst <= 1e-6


def test_device_tolerance_of_the_relative_covariance():
    e = BC.cov_reorder_error()
    print("float64 against long double on the relative covariance: e = %.3e; device bar %.3e" % (e, BC.device_cov_bar()))
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 here"
    assert e > 0 and BC.device_cov_bar() == max(10 * e, 1e-12)
    assert BC.device_cov_bar() <= 1e-9


def test_relative_covariance_covers_the_actual_error():
    """the covariance means what it says: over noisy corners the actual ref<-bundle error, whitened by the reported
    covariance, has a mean square per degree of freedom near 1 (between 0.3 and 3 over the posed pairs of the two other bundles x 6)"""
    import pose_cov_ref as PC
    _, p, c = BC.statement("camera", 16, sigma_px=0.2, noise=True)
    truth = BC.truth()
    rel = BR.relative_records(p, c, 2)
    chi = []
    for f, b in zip(*np.nonzero(rel["status"] == 0)):
        if b == 2:
            continue
        Tt = truth[f, 2] @ np.linalg.inv(truth[f, b])
        x = PC.pose_error(rel["T"][f, b][:3, :3], rel["T"][f, b][:3, 3], Tt[:3, :3], Tt[:3, 3])
        chi.append(x @ np.linalg.solve(rel["cov"][f, b], x) / 6)
    print("whitened relative-pose error, mean square per degree of freedom: %.2f over %d pairs" % (np.mean(chi), len(chi)))
    assert 0.3 <= np.mean(chi) <= 3.0


def test_from_map_round_trip():
    """cut the scene of one instant into bundles: bundle<-tag composed with the object's true pose (world<-origin tag) gives
    the scene back, the origin sits at the identity, the sizes are carried, and the cut is the layout up to the origin's pose"""
    sc = BC.scene()
    cut = BundleSet.from_map(sc, BC.GROUPS)
    lays = BC.layouts()
    assert len(cut) == 3 and [m.ids() for m in cut.maps] == BC.GROUPS
    for b, g in enumerate(BC.GROUPS):
        assert np.array_equal(cut[b][g[0]], np.eye(4))
        for i in g:
            assert np.abs(sc[g[0]] @ cut[b][i] - sc[i]).max() <= 1e-12 * np.abs(sc[i]).max()
            assert cut[b].size(i) == lays[b].size(i)
            assert np.abs(cut[b][i] - np.linalg.inv(lays[b][g[0]]) @ lays[b][i]).max() <= 1e-12 * 20
    assert cut.bundle_of(BC.STRAY_ID) is None and cut.bundle_of(9) == 1
    # another origin, records in place of a TagMap, and what is refused
    cut2 = BundleSet.from_map(sc.as_records(), BC.GROUPS, origins=[None, 9, 6])
    assert np.array_equal(cut2[1][9], np.eye(4)) and np.abs(sc[9] @ cut2[1][2] - sc[2]).max() <= 1e-12 * np.abs(sc[2]).max()
    assert cut2[1].size(9) == BC.SIZES[9]
    for bad in (dict(groups=[[5], [2, 40]]), dict(groups=[[5], []]), dict(groups=BC.GROUPS, origins=[5, 2, 7]), dict(groups=BC.GROUPS, origins=[5])):
        with pytest.raises(ValueError):
            BundleSet.from_map(sc, **bad)


def test_bundle_set(tmp_path):
    bs = BC.bundle_set()
    with pytest.raises(ValueError, match="tag id 9 is valid in bundles pallet and extra"):
        BundleSet(BC.layouts() + [TagMap({9: np.eye(4)})], ["tool", "pallet", "pad", "extra"])
    with pytest.raises(ValueError):
        BundleSet([])
    with pytest.raises(ValueError):
        BundleSet(BC.layouts(), ["a", "a", "b"])
    t = bs.table(BC.N_IDS)
    assert t.shape == (3, 12) and t.dtype == _lib.MAP_TAG_DTYPE and t.flags.c_contiguous
    assert [np.flatnonzero(r["valid"]).tolist() for r in t] == BC.GROUPS
    assert t["size"][0, 5] == 20.0 and t["size"][1, 9] == 6.0 and t["size"][2].max() == 0
    for b, m in enumerate(bs.maps):
        assert t[b, :m.n_ids].tobytes() == m.as_records().tobytes()
    assert bs.n_ids == 12 and bs.table().tobytes() == t.tobytes() and bs.table(20).shape == (3, 20) and bs.table(20)[:, :12].tobytes() == t.tobytes()
    assert bs.table(6)["valid"].sum() == 4                       # ids at or above n_ids are left out
    assert bs.index("pad") == 2 and bs["pallet"] is bs.maps[1]
    path = str(tmp_path / "bundles.npz")
    bs.save(path)
    back = BundleSet.load(path)
    assert back.names == bs.names and back.table().tobytes() == t.tobytes()


def test_bundle_result_surface():
    _, p, c = BC.statement("camera", 16)
    r = BundleResult(p, c, BC.bundle_set())
    assert r.T.shape == (5, 3, 4, 4) and r.status.tolist() == BC.expected_status().tolist() and r.cov.shape == (5, 3, 6, 6)
    rot, tr = r.pose_std()
    assert rot.shape == tr.shape == (5, 3, 3) and (rot[BC.meant_posed()] > 0).all() and not rot[~BC.meant_posed()].any()
    with pytest.raises(ValueError):
        BundleResult(p).pose_std()
    with pytest.raises(ValueError):
        r.relative("pad")                                        # no detector to run on
