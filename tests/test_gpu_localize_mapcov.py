"""Localisation that carries the map's joint covariance into the pose covariance, on the device (asl_localize_mapcov_*,
asl_localize_rig_mapcov_*: loc_map_term in k_localize.inc) against the NumPy statement (tests/localize_mapcov_ref.py)
evaluated at the device's own pose and active set.

Bar, per element: |C_gpu - C_ref|_ij <= 1200 eps kappa sqrt(C_ii C_jj), solver_checks.assert_cov_close's with the factor
doubled because A^-1 is applied twice (once on each side of Q), kappa the condition number of the Jacobi-scaled J^T J; every
compared pose must have 1200 eps kappa <= 1e-6 (asserted).  The pose record is the plain call's to the byte, a map
covariance without a block for any slot gives the _cov form's record to the byte, and a bad slot entry or block gives
status 3 with the pose untouched.  Shapes: 1 (the world tag alone), 2, 7, 8, 9, 24 and 256 active slots -- 8 x 8 = 64 pairs
fill one round of lanes, 256 slots are the 4 x 4 round pairs of 65,536 pairs -- a gated tag, a lens model, a two-camera rig."""
import numpy as np
import pytest

import localize_cases as LC
import localize_mapcov_cases as LMC
import localize_mapcov_ref as LMR
import localize_ref as LR
import map_cases as MC
import map_cov_cases as MCC
import pose_cov_ref as PC
import rig_cases as RC
import rig_ref
import solver_edge_cases as SEC
from aprilslam_amd import _lib
from solver_checks import EPS, dev_bytes

pytestmark = pytest.mark.gpu

SIGMA = 0.3
SLOT_COUNTS = (1, 2, 7, 8, 9, 24, 256)


def build_case(name):
    """dict(obs, rec, rig or None, K, dist, gate): obs (n_frames, max_tags), or a rig's (n_cams, n_frames, max_tags)"""
    if name.startswith("slots_"):
        n = int(name[6:])
        tags, rec = SEC._grid16()
        # few slots: a tilted camera close to the first nine tags of row 0 (far away, a handful of small tags leaves J^T J
        # too ill-conditioned for the bar's precondition); many: the whole 16 x 16 grid from 380 units
        cams = SEC.grid_cameras(1, 9, 2, d=150.0)[1:] if n <= 9 else SEC.grid_cameras(16, 16, 2)[1:]
        obs = SEC.frames(tags, cams, n)
        assert obs["id"][0].tolist() == list(range(n))
        return dict(obs=obs, rec=rec, rig=None, K=SEC.K, dist=None, gate=0.0)
    if name == "rig":
        c = RC.case("mixed_models")
        return dict(obs=c["obs"][:, :2], rec=c["rec"], rig=c["rig"], K=None, dist=None, gate=0.0)
    _, obs, rec, dist, gate = [c for c in LC.cpu_cases(SEC.K) if c[0] == name][0]
    return dict(obs=obs[:2], rec=rec, rig=None, K=SEC.K, dist=dist, gate=gate)


CASES = ["slots_%d" % n for n in SLOT_COUNTS] + ["gate", "dist5", "rig"]


def map_cov_for(case, seed=11):
    """(cov_slot, matrix) for the case's map: a dense random covariance over every id the frames hold but the lowest,
    which stands for the world tag and is exact"""
    ids = sorted({int(i) for i in case["obs"]["id"].ravel() if i >= 0})[1:]
    n = max(len(ids), 1)
    return LMC.cov_slot(ids, len(case["rec"])), LMC.random_spd(6 * n, np.random.default_rng(seed)), ids


def run(det, case, map_cov=None, sigma_px=SIGMA):
    if case["rig"] is not None:
        return det.localize_rig(case["obs"], case["rec"], case["rig"], LC.TAG_INNER, case["gate"], sigma_px=sigma_px, map_cov=map_cov)
    return det.localize(case["obs"], case["rec"], case["K"], case["dist"], LC.TAG_INNER, case["gate"], sigma_px=sigma_px, map_cov=map_cov)


def model_of(case):
    return rig_ref.RigModel(case["rig"]) if case["rig"] is not None else LR.OneCamera(LR.camera(case["K"], case["dist"]))


def rows_of(case, f):
    return case["obs"][:, f] if case["rig"] is not None else case["obs"][f]


@pytest.fixture(scope="module")
def results(gpu_detector):
    out = {}
    for name in CASES:
        case = build_case(name)
        slot, mat, ids = map_cov_for(case)
        out[name] = (case, slot, mat, ids, run(gpu_detector, case, (slot, mat)))
    return out


@pytest.mark.parametrize("name", CASES)
def test_matches_the_statement_at_the_device_pose(results, name):
    case, slot, mat, ids, (poses, covs) = results[name]
    model = model_of(case)
    for f in range(len(poses)):
        rows = rows_of(case, f)
        assert poses["status"][f] == 0 and covs["status"][f] == 0
        # the active set: the statement's own solve tells which slot the gate dropped; the device must have dropped as many
        _, _, active, trace = LR.solve_frame(model, rows, case["rec"], LC.TAG_INNER, case["gate"])
        assert poses["n_tags"][f] == len(active) and poses["n_rejected"][f] == len(trace["dropped"])
        if name == "gate":
            assert [int(rows.reshape(-1)["id"][s]) for s in trace["dropped"]] == [7]      # localize_cases moved tag 7
        T = poses["T"][f]
        R, t = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
        Xw, uv, ci = LR.frame_points(model, rows, case["rec"], LC.TAG_INNER, active)
        want = LMR.frame_cov(model, rows, case["rec"], LC.TAG_INNER, (R, t), active, SIGMA, slot, mat)
        assert want["status"] == 0 and covs["dof"][f] == want["dof"] and covs["sigma_px"][f] == SIGMA
        kappa = PC.scaled_condition(LMR.normal_matrix(model, R, t, Xw, uv, ci))
        tol = 1200 * EPS * kappa
        assert tol <= 1e-6, (name, f, kappa)
        got, ref = covs["cov"][f], want["cov"]
        s = np.sqrt(np.diag(ref))
        err = np.abs(got - ref) / np.outer(s, s)
        print(name, f, "slots", len(active), "kappa %.3g" % kappa, "error %.3g" % err.max(), "bar %.3g" % tol)
        assert err.max() <= tol, (name, f, err.max(), tol)
        assert np.array_equal(got, got.T)
        if name != "slots_1":     # the map's share is there: far more than the bar over the pixel-only covariance
            pix = LR.frame_cov(model, rows, case["rec"], LC.TAG_INNER, (R, t), active, SIGMA)["cov"]
            assert (np.abs(got - pix) / np.outer(s, s)).max() > 100 * tol


def test_a_gated_tag_does_not_contribute(gpu_detector, results):
    """tag 7, which the gate drops, gets a variance of 1e6 in the map covariance: the record must not move beyond rounding"""
    case, slot, mat, ids, (poses, covs) = results["gate"]
    big = mat.copy()
    k = ids.index(7)
    big[6 * k:6 * k + 6, 6 * k:6 * k + 6] += 1e6 * np.eye(6)
    poses2, covs2 = run(gpu_detector, case, (slot, big))
    assert poses2.tobytes() == poses.tobytes() and covs2.tobytes() == covs.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_pose_bytes_and_the_all_exact_record(gpu_detector, results, name):
    case, slot, mat, ids, (poses, covs) = results[name]
    plain = run(gpu_detector, case, sigma_px=None)
    assert poses.tobytes() == plain.tobytes()
    cov_form = run(gpu_detector, case)
    exact = run(gpu_detector, case, (np.full_like(slot, -1), mat))
    assert exact[0].tobytes() == cov_form[0].tobytes() and exact[1].tobytes() == cov_form[1].tobytes()
    if name == "slots_1":         # the world tag alone: no block, Q = 0
        assert covs.tobytes() == cov_form[1].tobytes()


@pytest.mark.parametrize("name", ["slots_9", "slots_256", "rig"])
def test_device_form_determinism_and_status_3(gpu_detector, results, name):
    import torch
    case, slot, mat, ids, (poses, covs) = results[name]
    dev = torch.device("cuda:0")
    obs, rec = case["obs"], np.ascontiguousarray(case["rec"])
    nf = obs.shape[-2]
    d_obs, d_map = dev_bytes(obs, dev), dev_bytes(rec, dev)
    d_rig = dev_bytes(_lib._rig_records(case["rig"]), dev) if case["rig"] is not None else None
    ld = mat.shape[1] + 12                                   # a leading dimension larger than the matrix
    wide = np.zeros((mat.shape[0], ld))
    wide[:, :mat.shape[1]] = mat

    def call(slot_a, mat_a):
        d_slot, d_mat = torch.from_numpy(np.ascontiguousarray(slot_a)).to(dev), torch.from_numpy(np.ascontiguousarray(mat_a)).to(dev)
        d_out = torch.zeros(nf * _lib.CAM_POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cov = torch.zeros(nf * _lib.POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        mc = (d_mat.data_ptr(), mat_a.shape[1], d_slot.data_ptr())
        if d_rig is not None:
            gpu_detector.localize_rig_device(d_obs.data_ptr(), obs.shape[0], nf, obs.shape[2], d_map.data_ptr(), len(rec), d_rig.data_ptr(),
                                             d_out.data_ptr(), LC.TAG_INNER, case["gate"], cov_ptr=d_cov.data_ptr(), sigma_px=SIGMA, map_cov=mc)
        else:
            gpu_detector.localize_device(d_obs.data_ptr(), nf, obs.shape[1], d_map.data_ptr(), len(rec), d_out.data_ptr(), case["K"], case["dist"],
                                         LC.TAG_INNER, case["gate"], cov_ptr=d_cov.data_ptr(), sigma_px=SIGMA, map_cov=mc)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(_lib.CAM_POSE_DTYPE), d_cov.cpu().numpy().view(_lib.POSE_COV_DTYPE)

    for _ in range(2):                                       # the host form's bytes, twice
        p, c = call(slot, wide)
        assert p.tobytes() == poses.tobytes() and c.tobytes() == covs.tobytes()
    every =[i for i in ids if all(i in (obs["id"][:, f] if obs.ndim == 3 else obs["id"][f]) for f in range(nf))]     # ids in view in every frame
    a, b = every[0], every[-1]
    bad = slot.copy()
    bad[b] = ld // 6                                         # one past the last block the leading dimension holds
    low = slot.copy()
    low[a] = -2
    nan = wide.copy()
    nan[6 * slot[b] + 1, 6 * slot[a] + 2] = np.nan           # inside the block (b, a)
    for s_a, m_a in ((bad, wide), (low, wide), (slot, nan)):
        p, c = call(s_a, m_a)
        assert p.tobytes() == poses.tobytes()
        assert (c["status"] == 3).all() and not c["cov"].any() and (c["dof"] == covs["dof"]).all()


def test_host_form_refuses_what_the_device_reports(gpu_detector, results):
    case, slot, mat, ids, _ = results["slots_9"]
    bad = slot.copy()
    bad[ids[0]] = mat.shape[1] // 6
    with pytest.raises(_lib.AslError, match="cov_slot"):
        run(gpu_detector, case, (bad, mat))
    nan = mat.copy()
    nan[3, 40] = np.inf
    with pytest.raises(_lib.AslError, match="not finite"):
        run(gpu_detector, case, (slot, nan))


def test_map_then_localise_on_one_stream(gpu_detector):
    """device map with its covariance -> device localisation that reads it, one stream, no host copy of the matrix; the
    records equal those of the host forms chained by hand"""
    import torch
    dev = torch.device("cuda:0")
    obs = np.ascontiguousarray(MCC.tag_count_block(9))
    nf, mt = obs.shape
    n_ids, cap = MC.N_IDS, 12
    K = MCC.MBC.K
    u8 = dict(dtype=torch.uint8, device=dev)
    d_obs = dev_bytes(obs, dev)
    d_map = torch.empty(n_ids * _lib.MAP_TAG_DTYPE.itemsize, **u8)
    d_std = torch.empty((n_ids, 6), dtype=torch.float64, device=dev)
    d_poses = torch.empty(nf * _lib.CAM_POSE_DTYPE.itemsize, **u8)
    d_res = torch.empty(_lib.MAP_RESULT_DTYPE.itemsize, **u8)
    d_slot = torch.empty(n_ids, dtype=torch.int32, device=dev)
    d_mat = torch.zeros((6 * cap, 6 * cap), dtype=torch.float64, device=dev)
    d_loc = torch.empty(nf * _lib.CAM_POSE_DTYPE.itemsize, **u8)
    d_cov = torch.empty(nf * _lib.POSE_COV_DTYPE.itemsize, **u8)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    gpu_detector.build_map_device(d_obs.data_ptr(), nf, mt, n_ids, K, None, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                                  d_res.data_ptr(), max_iters=60, stream=stream.cuda_stream, cov=(d_slot.data_ptr(), d_mat.data_ptr(), cap))
    gpu_detector.localize_device(d_obs.data_ptr(), nf, mt, d_map.data_ptr(), n_ids, d_loc.data_ptr(), K, None, LC.TAG_INNER, stream=stream.cuda_stream,
                                 cov_ptr=d_cov.data_ptr(), sigma_px=0.0, map_cov=(d_mat.data_ptr(), 6 * cap, d_slot.data_ptr()))
    stream.synchronize()
    res, tmap, std, mposes, (slot, mat) = gpu_detector.build_map(obs, n_ids, K, None, LC.TAG_INNER, max_iters=60, with_cov=True)
    assert res["status"] == 0 and (slot >= 0).sum() == 9
    assert d_map.cpu().numpy().tobytes() == tmap.tobytes() and d_slot.cpu().numpy().tobytes() == slot.tobytes()
    poses, covs = gpu_detector.localize(obs, tmap, K, None, LC.TAG_INNER, sigma_px=0.0, map_cov=(slot, mat))
    assert d_loc.cpu().numpy().tobytes() == poses.tobytes() and d_cov.cpu().numpy().tobytes() == covs.tobytes()
    plain = gpu_detector.localize(obs, tmap, K, None, LC.TAG_INNER, sigma_px=0.0)[1]
    assert (covs["status"] == 0).all()
    ratio = np.sqrt(np.diagonal(covs["cov"], axis1=1, axis2=2) / np.diagonal(plain["cov"], axis1=1, axis2=2))
    print("std with the map's covariance / pixel-only std, per frame:", ratio.min(axis=1), ratio.max(axis=1))
    assert (ratio > 1).all()
