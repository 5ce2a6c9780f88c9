"""Tag bundles on the device (asl_localize_bundles_* and asl_bundle_relative_*; the bundle dimension of k_localize.inc and
k_rig.inc, k_bundle.inc) on the inputs of tests/bundle_cases.py.

The localisation contract is byte equality: record (f, b) of the bundle call is what the one-map call writes for frame f
with table b alone.  The relative pose is held to the NumPy statement (tests/bundle_ref.py): T per entry within
16 eps (1 + |p_a| + |p_b|), the covariance within bundle_cases.device_cov_bar() (ten times what reordering float64 costs,
derived in tests/test_bundle_ref.py) per element over sqrt(C_ii C_jj), symmetric to the bit."""
import ctypes as C

import numpy as np
import pytest

import bundle_cases as BC
import bundle_ref as BR
import localize_cases as LC
from aprilslam_amd import _lib
from aprilslam_amd.bundles import BundleResult
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE
from solver_checks import dev_bytes

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KINDS = [("camera", mt) for mt in BC.MAX_TAGS] + [("rig", 4)]
# (name, noisy corners, sigma_px: None plain, gate)
VARIANTS = [("plain", False, None, 0.0), ("sigma", False, 0.5, 0.0), ("estimated", True, 0.0, 0.0), ("gated", True, 0.0, 0.25), ("plain_gated", True, None, 0.25)]


def block(kind, max_tags, noise):
    obs = BC.camera_block(max_tags) if kind == "camera" else BC.rig_block(max_tags)
    return np.ascontiguousarray(BC.noisy(obs) if noise else obs)


def frames(kind, obs, sl):
    return np.ascontiguousarray(obs[sl] if kind == "camera" else obs[:, sl])


def one_map(det, kind, obs, table, gate, sigma):
    """the existing call: (poses (n_frames,), cov (n_frames,) or None)"""
    if kind == "camera":
        got = det.localize(obs, table, BC.K, None, BC.TAG_SIZE, gate, sigma_px=sigma)
    else:
        got = det.localize_rig(obs, table, BC.rig_of_two(), BC.TAG_SIZE, gate, sigma_px=sigma)
    return got if sigma is not None else (got, None)


def bundle_host(det, kind, obs, tabs, gate, sigma):
    if kind == "camera":
        got = det.localize_bundles(obs, tabs, BC.K, None, BC.TAG_SIZE, gate, sigma_px=sigma)
    else:
        got = det.localize_bundles_rig(obs, tabs, BC.rig_of_two(), BC.TAG_SIZE, gate, sigma_px=sigma)
    return got if sigma is not None else (got, None)


def bundle_device(det, kind, obs, tabs, gate, sigma):
    """the device form on 0xAB-filled outputs: (poses bytes, cov bytes or None)"""
    import torch
    dev = torch.device("cuda:0")
    tabs = np.ascontiguousarray(tabs)
    nb, n_ids = tabs.shape
    nf, mt = obs.shape[-2:]
    d_obs, d_maps = dev_bytes(obs, dev), dev_bytes(tabs, dev)
    d_out = torch.full((nf * nb * CAM_POSE_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
    d_cov = torch.full((nf * nb * POSE_COV_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev) if sigma is not None else None
    st = torch.cuda.current_stream().cuda_stream
    cp = None if d_cov is None else d_cov.data_ptr()
    if kind == "camera":
        det.localize_bundles_device(d_obs.data_ptr(), nf, mt, d_maps.data_ptr(), nb, n_ids, d_out.data_ptr(), BC.K, None, BC.TAG_SIZE, gate, stream=st,
                                    cov_ptr=cp, sigma_px=sigma or 0.0)
    else:
        d_rig = dev_bytes(BC.rig_of_two().as_records(), dev)
        det.localize_bundles_rig_device(d_obs.data_ptr(), obs.shape[0], nf, mt, d_maps.data_ptr(), nb, n_ids, d_rig.data_ptr(), d_out.data_ptr(),
                                        BC.TAG_SIZE, gate, stream=st, cov_ptr=cp, sigma_px=sigma or 0.0)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes(), None if d_cov is None else d_cov.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind,max_tags", KINDS)
def test_records_are_the_one_map_calls_bytes(gpu_detector, kind, max_tags):
    """host and device forms, n_bundles 3 and 1, n_frames 5 and 1, over the variants (plain, sigma given, sigma estimated on
    noisy corners, gate off and on)"""
    tabs = BC.tables()
    rejected = 0
    for name, noise, sigma, gate in VARIANTS:
        obs = block(kind, max_tags, noise)
        want = [one_map(gpu_detector, kind, obs, tabs[b], gate, sigma) for b in range(3)]
        wp = np.stack([w[0] for w in want], axis=1)
        wc = None if sigma is None else np.stack([w[1] for w in want], axis=1)
        assert wp["status"].tolist() == BC.expected_status().tolist(), name
        rejected += int(wp["n_rejected"].sum())
        gp, gc = bundle_host(gpu_detector, kind, obs, tabs, gate, sigma)
        assert gp.shape == (BC.N_FRAMES, 3) and gp.tobytes() == wp.tobytes(), name
        assert (gc is None) == (wc is None) and (gc is None or gc.tobytes() == wc.tobytes()), name
        dp, dc = bundle_device(gpu_detector, kind, obs, tabs, gate, sigma)
        assert dp == wp.tobytes() and (dc is None or dc == wc.tobytes()), name
        for b in range(3):                                       # n_bundles = 1: each table alone
            p1, c1 = bundle_host(gpu_detector, kind, obs, tabs[b:b + 1], gate, sigma)
            assert p1.shape == (BC.N_FRAMES, 1) and p1.tobytes() == wp[:, b].tobytes() and (c1 is None or c1.tobytes() == wc[:, b].tobytes()), (name, b)
        for f in (1, 3):                                         # n_frames = 1: the frames with a status of their own
            pf, cf = bundle_host(gpu_detector, kind, frames(kind, obs, slice(f, f + 1)), tabs, gate, sigma)
            assert pf.tobytes() == wp[f].tobytes() and (cf is None or cf.tobytes() == wc[f].tobytes()), (name, f)
            dp, dc = bundle_device(gpu_detector, kind, frames(kind, obs, slice(f, f + 1)), tabs[1:2], gate, sigma)
            assert dp == wp[f, 1].tobytes() and (dc is None or dc == wc[f, 1].tobytes()), (name, f)
    print(kind, max_tags, "slots dropped by the gate over the gated variants:", rejected)
    assert rejected > 0                                          # the gate acted where it was on


@pytest.mark.parametrize("kind,max_tags", KINDS)
def test_plain_poses_are_the_covariance_calls_and_calls_repeat(gpu_detector, kind, max_tags):
    tabs = BC.tables()
    obs = block(kind, max_tags, True)
    plain, _ = bundle_host(gpu_detector, kind, obs, tabs, 0.25, None)
    with_cov, cov = bundle_host(gpu_detector, kind, obs, tabs, 0.25, 0.0)
    assert plain.tobytes() == with_cov.tobytes()
    again, cov2 = bundle_host(gpu_detector, kind, obs, tabs, 0.25, 0.0)
    assert again.tobytes() == with_cov.tobytes() and cov2.tobytes() == cov.tobytes()
    d1, d2 = bundle_device(gpu_detector, kind, obs, tabs, 0.25, 0.0), bundle_device(gpu_detector, kind, obs, tabs, 0.25, 0.0)
    assert d1 == d2 == (with_cov.tobytes(), cov.tobytes())
    rel = [gpu_detector.bundle_relative(with_cov, cov, 2).tobytes() for _ in range(2)]
    assert rel[0] == rel[1]


def relative_device(det, poses, cov, ref):
    import torch
    dev = torch.device("cuda:0")
    nf, nb = poses.shape
    d_p = dev_bytes(poses, dev)
    d_c = None if cov is None else dev_bytes(cov, dev)
    d_rel = torch.full((nf * nb * _lib.BUNDLE_REL_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=dev)
    det.bundle_relative_device(d_p.data_ptr(), None if d_c is None else d_c.data_ptr(), nf, nb, ref, d_rel.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_rel.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind,max_tags", KINDS)
def test_relative_pose_against_the_statement(gpu_detector, kind, max_tags):
    """on the device's own poses and covariances of the case, ref = 0 and ref = last"""
    bar = BC.device_cov_bar()
    p, c = bundle_host(gpu_detector, kind, block(kind, max_tags, False), BC.tables(), 0.0, BC.SIGMA)
    no_cov = c.copy()
    no_cov["status"][4, 1], no_cov["cov"][4, 1] = 2, 0           # one covariance with a status of its own
    worst_T = worst_C = 0.0
    for ref in (0, 2):
        for cov in (c, None, no_cov):
            got = gpu_detector.bundle_relative(p, cov, ref)
            want = BR.relative_records(p, cov, ref)
            assert got.shape == (BC.N_FRAMES, 3) and got["status"].tolist() == want["status"].tolist() and not got["reserved"].any()
            assert relative_device(gpu_detector, p, cov, ref) == got.tobytes()
            for f in range(BC.N_FRAMES):
                for b in range(3):
                    g, w = got[f, b], want[f, b]
                    if w["status"] == 1 or b == ref:
                        assert np.array_equal(g["T"], np.eye(4)) and not g["cov"].any(), (ref, f, b)
                        continue
                    tol = 16 * EPS * (1 + np.linalg.norm(p["T"][f, ref][:3, 3]) + np.linalg.norm(p["T"][f, b][:3, 3]))
                    worst_T = max(worst_T, np.abs(g["T"] - w["T"]).max() / tol)
                    assert np.abs(g["T"] - w["T"]).max() <= tol, (ref, f, b)
                    assert g["T"][3].tolist() == [0, 0, 0, 1]
                    if w["status"] == 2:
                        assert not g["cov"].any(), (ref, f, b)
                        continue
                    s = np.sqrt(np.diag(w["cov"]))
                    err = (np.abs(g["cov"] - w["cov"]) / np.outer(s, s)).max()
                    worst_C = max(worst_C, err)
                    assert err <= bar, (ref, f, b, err, bar)
                    assert np.array_equal(g["cov"], g["cov"].T), (ref, f, b)
        assert (BR.relative_records(p, None, ref)["status"] == 2).any() and (BR.relative_records(p, no_cov, ref)["status"][4] == 2).any()
    print(kind, max_tags, "relative pose against the statement: T at %.2f of its bar, covariance off by %.2e (bar %.2e)" % (worst_T, worst_C, bar))


def test_python_layers(gpu_detector):
    """Rig.localize_bundles and BundleResult.relative over the same calls"""
    bs = BC.bundle_set()
    obs = block("rig", 4, False)
    res = BC.rig_of_two().localize_bundles(gpu_detector, obs, bs, BC.TAG_SIZE, with_cov=True, sigma_px=BC.SIGMA)
    p, c = bundle_host(gpu_detector, "rig", obs, BC.tables(), 0.0, BC.SIGMA)
    assert isinstance(res, BundleResult) and res.poses.tobytes() == p.tobytes() and res.cov_records.tobytes() == c.tobytes()
    assert res.relative("pad").tobytes() == gpu_detector.bundle_relative(p, c, 2).tobytes()
    truth = BC.truth(True)
    rel = res.relative("tool")
    for f, b in zip(*np.nonzero(rel["status"] == 0)):
        assert LC.rel_err(rel["T"][f, b], truth[f, 0] @ np.linalg.inv(truth[f, b])) <= 1e-6
    plain = BC.rig_of_two().localize_bundles(gpu_detector, obs, bs, BC.TAG_SIZE)
    assert plain.cov is None and plain.poses.tobytes() == p.tobytes() and (plain.relative(0)["status"][0] == [0, 2, 2]).all()


def test_refusals_write_nothing(gpu_detector):
    """n_bundles 0 and 1025, n_frames * n_bundles past int32, ref out of range, NULL maps, and max_tags 0 as the one-map calls'
    representative: -1 with a message, the pattern in every output intact, host and device forms"""
    import torch
    dev = torch.device("cuda:0")
    L = _lib.load()
    tabs = np.ascontiguousarray(BC.tables())
    Kc = np.ascontiguousarray(BC.K)
    Kp = Kc.ctypes.data_as(C.POINTER(C.c_double))
    rig = BC.rig_of_two().as_records()
    nf, nb = BC.N_FRAMES, 3
    blocks = {"camera": block("camera", 4, False), "rig": block("rig", 4, False)}
    poses, cov = bundle_host(gpu_detector, "camera", blocks["camera"], tabs, 0.0, BC.SIGMA)
    bad = [dict(n_bundles=0), dict(n_bundles=1025), dict(n_bundles=1024, n_frames=2097152), dict(maps=None), dict(max_tags=0)]
    bad_rel = [dict(n_bundles=0), dict(n_bundles=1025), dict(n_bundles=1024, n_frames=2097152), dict(ref=-1), dict(ref=3), dict(poses=None)]
    keep = []
    for device in (False, True):
        def mem(a):
            if device:
                keep.append(dev_bytes(a, dev))
                return keep[-1].data_ptr()
            keep.append(np.ascontiguousarray(a))
            return keep[-1].ctypes.data

        def pattern(nbytes):
            if device:
                return torch.full((nbytes,), 0x55, dtype=torch.uint8, device=dev)
            return np.full(nbytes, 0x55, dtype=np.uint8)

        def addr(buf):
            return buf.data_ptr() if device else buf.ctypes.data

        def intact(buf):
            if device:
                torch.cuda.synchronize()
            return bool((buf == 0x55).all())

        out, cv, rel = pattern(nf * nb * 160), pattern(nf * nb * 304), pattern(nf * nb * 424)
        for kind in ("camera", "rig"):
            ok = dict(obs=mem(blocks[kind]), n_frames=nf, max_tags=4, maps=mem(tabs), n_bundles=nb)
            for with_cov in (False, True):
                for b in bad:
                    a = dict(ok, **b)
                    tail = (BC.TAG_SIZE, 0.0, 0.5, addr(out), addr(cv) if with_cov else None) + ((None,) if device else ())
                    if kind == "camera":
                        fn = L.asl_localize_bundles_frames_device if device else L.asl_localize_bundles_batch
                        rc = fn(gpu_detector._h, a["obs"], a["n_frames"], a["max_tags"], a["maps"], a["n_bundles"], BC.N_IDS, Kp, None, 0, *tail)
                    else:
                        fn = L.asl_localize_bundles_rig_frames_device if device else L.asl_localize_bundles_rig_batch
                        rc = fn(gpu_detector._h, a["obs"], 2, a["n_frames"], a["max_tags"], a["maps"], a["n_bundles"], BC.N_IDS, mem(rig), *tail)
                    assert rc == -1 and len(L.asl_last_error()) > 0, (device, kind, with_cov, b)
        ok = dict(poses=mem(poses), cov=mem(cov), n_frames=nf, n_bundles=nb, ref=0)
        for b in bad_rel:
            a = dict(ok, **b)
            args = (gpu_detector._h, a["poses"], a["cov"], a["n_frames"], a["n_bundles"], a["ref"])
            rc = L.asl_bundle_relative_device(*args, addr(rel), None) if device else L.asl_bundle_relative_batch(*args, addr(rel))
            assert rc == -1 and len(L.asl_last_error()) > 0, (device, b)
        h = gpu_detector._h                                      # no room for the result
        assert (L.asl_bundle_relative_device(h, ok["poses"], ok["cov"], nf, nb, 0, None, None) if device else
                L.asl_bundle_relative_batch(h, ok["poses"], ok["cov"], nf, nb, 0, None)) == -1
        assert intact(out) and intact(cv) and intact(rel), device
    with pytest.raises(_lib.AslError, match="n_bundles"):
        gpu_detector.localize_bundles(blocks["camera"], np.zeros((1025, 2), dtype=_lib.MAP_TAG_DTYPE), BC.K, None, BC.TAG_SIZE)
    with pytest.raises(_lib.AslError, match="ref"):
        gpu_detector.bundle_relative(poses, cov, 3)


@pytest.mark.parametrize("case", ["exact", "mirrored", "gate", "gate_off", "slots", "dist4", "dist5"])
def test_existing_entry_points_are_unchanged(gpu_detector, case):
    """asl_localize_batch on localize_cases.cpu_cases, whose kernels now carry the bundle dimension, is the n_bundles = 1
    bundle call to the byte (and its covariance form with it)"""
    from aprilslam_amd import synth
    K = synth.camera_matrix(LC.W, LC.H, 45.0)
    name, obs, rec, dist, gate = [c for c in LC.cpu_cases(K) if c[0] == case][0]
    want = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    got = gpu_detector.localize_bundles(obs, rec[None], K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    assert got.shape == (len(obs), 1) and got[:, 0].tobytes() == want.tobytes()
    wp, wc = gpu_detector.localize(obs, rec, K, dist, LC.TAG_INNER, max_tag_rms_px=gate, sigma_px=0.5)
    gp, gc = gpu_detector.localize_bundles(obs, rec[None], K, dist, LC.TAG_INNER, max_tag_rms_px=gate, sigma_px=0.5)
    assert wp.tobytes() == want.tobytes() and gp[:, 0].tobytes() == wp.tobytes() and gc[:, 0].tobytes() == wc.tobytes()
    # two copies of the map as two bundles: both columns are the one-map call
    two = gpu_detector.localize_bundles(obs, np.stack([rec, rec]), K, dist, LC.TAG_INNER, max_tag_rms_px=gate)
    assert two[:, 0].tobytes() == want.tobytes() and two[:, 1].tobytes() == want.tobytes()
