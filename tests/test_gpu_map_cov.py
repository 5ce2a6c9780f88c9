"""The joint covariance of a reconstructed map on the device (asl_mapcov_*, asl_mapcov_rig_*: k_map_cols, k_map_cov_gram)
against the NumPy statement (tests/map_cov_ref.py) evaluated at the device's own solution.

Bars: element-wise |C_gpu - C_ref|_ij <= 1e-5 sqrt(C_ii C_jj) -- test_gpu_map.py's bar on the tag std (rtol 1e-5),
normalised so that near-zero off-diagonal entries are held too; sqrt of the diagonal against the call's own tag_std to
1e-12 relative (the same columns of L^-1, summed in another order: n eps with n <= 6000); every other output the bytes of
the call without the covariance; the same bytes again on a second call and from the device-pointer form."""
import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_cov_cases as MCC
import map_cov_ref as MCR
from aprilslam_amd import _lib
from aprilslam_amd.mapping import MapCovariance

pytestmark = pytest.mark.gpu

COV_TOL = 1e-5
DIAG_TOL = 1e-12


def build(det, case, with_cov, **kw):
    obs, rig, dist, huber, sizes = MCC.cases()[case]
    args = dict(huber_px=huber, with_slot_weight=True, tag_sizes=sizes, max_iters=60, with_cov=with_cov, **kw)
    if rig is not None:
        return det.build_map_rig(obs, MC.N_IDS, rig, LC.TAG_INNER, **args)
    return det.build_map(obs, MC.N_IDS, MBC_K, dist, LC.TAG_INNER, **args)


MBC_K = MCC.MBC.K


@pytest.fixture(scope="module")
def results(gpu_detector):
    """every case's covariance call, once"""
    return {name: build(gpu_detector, name, True) for name in MCC.cases()}


def statement(case, out):
    obs, rig, dist, huber, _ = MCC.cases()[case]
    res, tmap, std, poses, weight = out[:5]
    if rig is not None:
        return MCR.map_rig_cov(obs, rig, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]), huber)
    return MCR.map_cov(obs, MBC_K, dist, LC.TAG_INNER, tmap, poses, weight, int(res["world_id"]), huber)


@pytest.mark.parametrize("case", [c for c in MCC.cases() if c != "nothing"])
def test_matrix_matches_the_statement_at_the_device_solution(results, case):
    out = results[case]
    res, tmap, std = out[0], out[1], out[2]
    slot, C = out[5]
    ids, got = MCR.from_slots(slot, C)
    want_ids, want, s2 = statement(case, out)
    w = int(res["world_id"])
    assert res["status"] == 0 and s2 > 0
    assert ids == want_ids == [int(i) for i in np.flatnonzero(tmap["valid"]) if i != w]
    assert len(ids) == res["n_tags"] - 1 and C.shape == (6 * len(ids), 6 * len(ids))
    if case.startswith("tags_"):
        assert len(ids) == int(case[5:])
    assert np.array_equal(got, got.T)                                      # symmetric to the bit
    d = np.sqrt(np.diag(want))
    err = np.abs(got - want) / np.outer(d, d)
    print(case, "n_cov", len(ids), "max normalised error", err.max())
    assert err.max() <= COV_TOL, (case, err.max())
    own = np.concatenate([std[i] for i in ids])
    assert (own > 0).all()
    derr = np.abs(np.sqrt(np.diag(got)) / own - 1).max()
    print(case, "diagonal against tag_std", derr)
    assert derr <= DIAG_TOL, (case, derr)


def test_a_tag_without_a_view_has_no_block(results):
    obs = MCC.cases()["behind"][0]
    res, tmap = results["behind"][:2]
    slot = results["behind"][5][0]
    seen = sorted({int(i) for i in obs["id"].ravel() if i >= 0})
    victim = seen[-1]
    assert res["n_obs_dropped"] == 1 and not tmap["valid"][victim] and slot[victim] == -1
    assert sorted(int(i) for i in np.flatnonzero(slot >= 0)) == seen[1:-1]


def test_a_failed_solve_has_no_covariance(results):
    out = results["nothing"]
    assert out[0]["status"] == 1
    assert (out[5][0] == -1).all() and out[5][1].shape == (0, 0)


@pytest.mark.parametrize("case", ["tags_1", "tags_9", "behind", "huber_dist5", "sized", "rig_pair", "nothing"])
def test_every_other_output_is_the_sized_calls(gpu_detector, results, case):
    plain = build(gpu_detector, case, False)
    assert len(plain) == 5
    for k, (a, b) in enumerate(zip(plain, results[case][:5])):
        assert a.tobytes() == b.tobytes(), (case, k)


@pytest.mark.parametrize("case", ["tags_8", "tags_17", "rig_pair"])
def test_the_same_input_gives_the_same_bytes(gpu_detector, results, case):
    again = build(gpu_detector, case, True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:5], results[case][:5]))
    assert again[5][0].tobytes() == results[case][5][0].tobytes() and again[5][1].tobytes() == results[case][5][1].tobytes()


@pytest.mark.parametrize("case", ["tags_9", "rig_pair"])
def test_device_pointer_form(gpu_detector, results, case):
    """the device form writes the host form's bytes into the leading region of a larger matrix and nothing beyond it"""
    import torch

    from solver_checks import dev_bytes
    obs, rig, dist, huber, sizes = MCC.cases()[case]
    dev = torch.device("cuda:0")
    want = results[case]
    n_cov = int((want[5][0] >= 0).sum())
    cap = n_cov + 3
    nf = obs.shape[-2]
    d_obs = dev_bytes(obs, dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    d_map = torch.empty(MC.N_IDS * _lib.MAP_TAG_DTYPE.itemsize, **u8)
    d_std = torch.empty((MC.N_IDS, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty(nf * _lib.CAM_POSE_DTYPE.itemsize, **u8)
    d_res = torch.empty(_lib.MAP_RESULT_DTYPE.itemsize, **u8)
    d_w = torch.empty(obs.shape, dtype=torch.float64, device=dev)
    d_slot = torch.full((MC.N_IDS,), 77, dtype=torch.int32, device=dev)
    d_cov = torch.full((6 * cap, 6 * cap), 7.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    outs = (d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(), d_res.data_ptr())
    kw = dict(max_iters=60, stream=stream.cuda_stream, huber_px=huber, slot_weight_ptr=d_w.data_ptr(), tag_sizes=sizes,
              cov=(d_slot.data_ptr(), d_cov.data_ptr(), cap))
    if rig is not None:
        d_rig = dev_bytes(_lib._rig_records(rig), dev)
        gpu_detector.build_map_rig_device(d_obs.data_ptr(), obs.shape[0], nf, obs.shape[2], MC.N_IDS, d_rig.data_ptr(), LC.TAG_INNER, *outs, **kw)
    else:
        gpu_detector.build_map_device(d_obs.data_ptr(), nf, obs.shape[1], MC.N_IDS, MBC_K, dist, LC.TAG_INNER, *outs, **kw)
    stream.synchronize()
    assert d_res.cpu().numpy().tobytes() == want[0].tobytes() and d_map.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_std.cpu().numpy().tobytes() == want[2].tobytes() and d_poses.cpu().numpy().tobytes() == want[3].tobytes()
    assert d_w.cpu().numpy().tobytes() == want[4].tobytes()
    assert d_slot.cpu().numpy().tobytes() == want[5][0].tobytes()
    M = d_cov.cpu().numpy()
    n = 6 * n_cov
    assert M[:n, :n].tobytes() == want[5][1].tobytes()
    assert (M[n:, :] == 7.0).all() and (M[:, n:] == 7.0).all()


def test_more_tags_than_cap_tags_is_refused_after_the_wait(gpu_detector):
    """9 tags besides the world tag into cap_tags 8: ASL_EINVAL once the sizes are known, and no output is written"""
    obs = np.ascontiguousarray(MCC.tag_count_block(9))
    nf, mt = obs.shape
    res = np.full(_lib.MAP_RESULT_DTYPE.itemsize, 0x55, dtype=np.uint8)
    tm = np.full(MC.N_IDS * _lib.MAP_TAG_DTYPE.itemsize, 0x55, dtype=np.uint8)
    poses = np.full(nf * _lib.CAM_POSE_DTYPE.itemsize, 0x55, dtype=np.uint8)
    slot = np.full(MC.N_IDS, 0x55555555, dtype=np.int32)
    Kc = np.ascontiguousarray(MBC_K)

    def call(cap):
        mat = np.full((6 * cap, 6 * cap), 7.0)
        rc = gpu_detector._L.asl_mapcov_batch(gpu_detector._h, obs.ctypes.data, nf, mt, MC.N_IDS, Kc.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)), None, 0,
                                               LC.TAG_INNER, None, -1, 0.0, 30, tm.ctypes.data, None, poses.ctypes.data, res.ctypes.data, None,
                                               slot.ctypes.data, mat.ctypes.data, cap)
        return rc, mat
    rc, mat = call(8)
    assert rc == -1 and b"9 tags besides the world tag" in gpu_detector._L.asl_last_error()
    assert (res == 0x55).all() and (tm == 0x55).all() and (poses == 0x55).all() and (slot == 0x55555555).all() and (mat == 7.0).all()
    rc, mat = call(9)
    assert rc == 0 and (slot >= 0).sum() == 9 and not (mat == 7.0).any()


def test_map_covariance_object(results, tmp_path):
    out = results["tags_7"]
    cov = MapCovariance.from_slots(*out[5])
    ids = [int(i) for i in np.flatnonzero(out[5][0] >= 0)]
    assert cov.ids == ids and cov.matrix.shape == (42, 42)
    assert np.array_equal(cov.block(ids[1], ids[3]), out[5][1][6:12, 18:24]) and np.array_equal(cov.block(ids[3], ids[1]), cov.block(ids[1], ids[3]).T)
    assert np.array_equal(cov.marginal(ids[2]), out[5][1][12:18, 12:18])
    np.testing.assert_allclose(cov.std(ids[2]), out[2][ids[2]], rtol=DIAG_TOL)
    p = str(tmp_path / "cov.npz")
    cov.save_npz(p)
    back = MapCovariance.load_npz(p)
    assert back.ids == cov.ids and back.matrix.tobytes() == cov.matrix.tobytes()
