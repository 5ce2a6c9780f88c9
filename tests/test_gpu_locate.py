"""Tag location on the device (asl_locate_tags_frames_device / asl_locate_tags_batch, k_locate.inc) against the NumPy
statement (tests/locate_ref.py) on every case of tests/locate_cases.py, and as one device chain on rendered frames:
localise against half the map, locate the other half, localise again against the extended map."""
import ctypes as C
import functools

import numpy as np
import pytest

import locate_cases as QC
import locate_ref as QR
import localize_cases as LC
from aprilslam_amd import _lib
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap

pytestmark = pytest.mark.gpu

K = QC.K
T_TOL = 1e-9   # relative, every case: the noise case needs no allowance for a trial decided the other way (measured: at most 2.2e-10)


@functools.lru_cache(maxsize=None)
def statement(name):
    _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
    traces = {}
    out = QR.locate_tags(obs, poses, map_in, K, dist, QC.TAG, gate, min_views, sigma_px=0.0, traces=traces)
    return out, traces


def assert_same(name, got, want, traces, map_in, tol):
    (gm, gf, gc), (wm, wf, wc) = got, want
    for i in range(len(wf)):
        g, w = gf[i], wf[i]
        for k in ("status", "n_views", "n_rejected", "seed_mirrored"):
            assert g[k] == w[k], (name, i, k, g[k], w[k])
        assert gc["status"][i] == wc["status"][i] and gc["dof"][i] == wc["dof"][i], (name, i)
        if w["status"] != 0:
            assert g["seed_frame"] == -1 and g["rms_px"] == 0 and g["rms_seed_px"] == 0
            assert gm[i].tobytes() == map_in[i].tobytes(), (name, i)          # not located: the entry keeps its bytes
            assert not gc["cov"][i].any()
            continue
        if g["seed_frame"] != w["seed_frame"]:                               # a candidate of equal score
            tv, trace = traces[i][0], traces[i][1]
            sc = {(tv.views[v][0], m): c for v, m, c in trace["first"]}
            a, b = sc[(int(g["seed_frame"]), int(g["seed_mirrored"]))], sc[(int(w["seed_frame"]), int(w["seed_mirrored"]))]
            assert abs(a - b) <= 1e-9 * max(1.0, b), (name, i, g["seed_frame"], w["seed_frame"])
        err = LC.rel_err(gm["T"][i], wm["T"][i])
        print("%s id %d: T rel err %.3g" % (name, i, err))
        assert err <= tol, (name, i, err)
        assert gm["valid"][i] == 1 and gm["size"][i].tobytes() == map_in["size"][i].tobytes()
        assert abs(g["rms_px"] - w["rms_px"]) <= 1e-6 * max(1.0, w["rms_px"]), (name, i)
        assert abs(g["rms_seed_px"] - w["rms_seed_px"]) <= 1e-6 * max(1.0, w["rms_seed_px"]), (name, i)
        assert np.array_equal(gc["cov"][i], gc["cov"][i].T)
        if wc["status"][i] == 0:
            assert np.abs(gc["cov"][i] - wc["cov"][i]).max() <= 1e-6 * np.abs(wc["cov"][i]).max(), (name, i)
            assert abs(gc["sigma_px"][i] - wc["sigma_px"][i]) <= 1e-6 * max(1.0, wc["sigma_px"][i])


@pytest.mark.parametrize("name", QC.CASES)
def test_kernel_matches_the_statement(gpu_detector, name):
    _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
    want, traces = statement(name)
    before = map_in.copy()
    got = gpu_detector.locate_tags(obs, poses, map_in, K, dist, QC.TAG, max_view_rms_px=gate, min_views=min_views, sigma_px=0.0)
    assert map_in.tobytes() == before.tobytes()                               # the caller's block is not modified
    assert_same(name, got, want, traces, map_in, T_TOL)
    plain = gpu_detector.locate_tags(obs, poses, map_in, K, dist, QC.TAG, max_view_rms_px=gate, min_views=min_views)
    assert plain[2] is None and plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()


def _device_call(det, torch, obs, poses, map_in, dist, gate, min_views, with_cov):
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    d_obs, d_poses, d_map = up(obs), up(poses), up(map_in)
    d_fit = torch.zeros(len(map_in) * _lib.TAG_FIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cov = torch.zeros(len(map_in) * POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev) if with_cov else None
    det.locate_tags_device(d_obs.data_ptr(), obs.shape[0], obs.shape[1], d_poses.data_ptr(), d_map.data_ptr(), len(map_in), d_fit.data_ptr(),
                           K, dist, QC.TAG, max_view_rms_px=gate, min_views=min_views, stream=torch.cuda.current_stream().cuda_stream,
                           cov_ptr=d_cov.data_ptr() if with_cov else None, sigma_px=0.0)
    torch.cuda.synchronize()
    return d_map.cpu().numpy().tobytes(), d_fit.cpu().numpy().tobytes(), d_cov.cpu().numpy().tobytes() if with_cov else None


def test_host_form_and_device_form_give_identical_bytes(gpu_detector):
    import torch
    _, obs, poses, map_in, dist, gate, min_views = QC.case("exact")
    m, fit, cov = gpu_detector.locate_tags(obs, poses, map_in, K, dist, QC.TAG, max_view_rms_px=gate, min_views=min_views, sigma_px=0.0)
    dm, dfit, dcov = _device_call(gpu_detector, torch, obs, poses, map_in, dist, gate, min_views, True)
    assert dm == m.tobytes() and dfit == fit.tobytes() and dcov == cov.tobytes()


def test_ten_repeats_give_identical_bytes(gpu_detector):
    import torch
    _, obs, poses, map_in, dist, gate, min_views = QC.case("gate_cap")       # the longest path: re-seeds up to the cap
    first = None
    for _ in range(10):
        got = _device_call(gpu_detector, torch, obs, poses, map_in, dist, gate, min_views, True)     # the map uploaded afresh
        first = got if first is None else first
        assert got == first


@pytest.fixture(scope="module")
def device_chain():
    """256 bench frames rendered on the device -> detect + PnP -> asl_obs records -> localisation against the even ids ->
    location of the odd ids -> localisation of the same block against the extended map: one stream, one read-back"""
    import torch

    import bench
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    n, max_tags = 256, 32
    frames, _, _ = bench.render_stream_device(det, n, dev)
    full = TagMap.from_scene(LC.bench_scene()).as_records()
    rec = full.copy()
    rec[1::2] = np.zeros((), dtype=_lib.MAP_TAG_DTYPE)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    d_obs = torch.empty((n, max_tags, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_first = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_second = torch.empty((n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_fit = torch.empty((len(rec), _lib.TAG_FIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    det.submit_device(frames.data_ptr(), n, 3, LC.W, LC.H, stream=s, K=K, dist=np.zeros(4), tag_size=LC.TAG_INNER)
    det.pack_observations_device(d_obs.data_ptr(), max_tags, stream=s)
    det.localize_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), len(rec), d_first.data_ptr(), K, None, LC.TAG_INNER, stream=s)
    det.locate_tags_device(d_obs.data_ptr(), n, max_tags, d_first.data_ptr(), d_map.data_ptr(), len(rec), d_fit.data_ptr(), K, None, LC.TAG_INNER,
                           max_view_rms_px=QC.GATE, stream=s)
    det.localize_device(d_obs.data_ptr(), n, max_tags, d_map.data_ptr(), len(rec), d_second.data_ptr(), K, None, LC.TAG_INNER, stream=s)
    stream.synchronize()
    first = d_first.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    second = d_second.cpu().numpy().view(CAM_POSE_DTYPE).reshape(n)
    fit = d_fit.cpu().numpy().view(_lib.TAG_FIT_DTYPE).reshape(len(rec))
    out = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(len(rec))
    det.collect()
    yield rec, full, out, fit, first, second
    det.close()


def test_device_chain_extends_the_map_and_the_frames_use_it(device_chain):
    rec, full, out, fit, first, second = device_chain
    odd = np.arange(1, len(rec), 2)
    assert (fit["status"][odd] == 0).all() and (fit["status"][::2] == 1).all()
    assert out[::2].tobytes() == rec[::2].tobytes() and (out["valid"] == 1).all()
    assert (first["status"] == 0).all() and (second["status"] == 0).all()
    assert (second["n_tags"] > first["n_tags"]).all()
    assert (second["rms_px"] < 1.0).all()
    for i in odd:
        T = np.vstack([full["T"][i].reshape(3, 4), [0, 0, 0, 1]])
        dp, dr = QC.pose_errors(out["T"][i], T)
        print("id %d: %d views, %d rejected, rms %.3f px, %.3f units and %.3f mrad from the scene" % (i, fit["n_views"][i], fit["n_rejected"][i], fit["rms_px"][i], dp, dr * 1e3))
        assert fit["rms_px"][i] < 1.0


def test_refusals_touch_no_output(gpu_detector):
    import torch
    dev = torch.device("cuda:0")
    _, obs, poses, map_in, _, _, _ = QC.case("exact")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    d_obs, d_poses, d_map = up(obs), up(poses), up(map_in)
    d_fit = torch.full((len(map_in) * 40,), 0xAB, dtype=torch.uint8, device=dev)
    d_cov = torch.full((len(map_in) * 304,), 0xAB, dtype=torch.uint8, device=dev)
    ok = dict(obs_ptr=d_obs.data_ptr(), n_frames=obs.shape[0], max_tags=obs.shape[1], poses_ptr=d_poses.data_ptr(), map_ptr=d_map.data_ptr(),
              n_ids=len(map_in), fit_ptr=d_fit.data_ptr(), K=K, dist=None, tag_size=QC.TAG, max_view_rms_px=0.0, min_views=2,
              cov_ptr=d_cov.data_ptr(), sigma_px=0.0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(obs_ptr=0), dict(poses_ptr=0), dict(map_ptr=0), dict(fit_ptr=0), dict(n_frames=-1), dict(max_tags=0), dict(max_tags=257),
           dict(n_ids=0), dict(tag_size=0.0), dict(tag_size=-1.0), dict(tag_size=nan), dict(max_view_rms_px=-0.5), dict(max_view_rms_px=nan),
           dict(max_view_rms_px=inf), dict(min_views=0), dict(min_views=-3), dict(sigma_px=-1.0), dict(sigma_px=nan), dict(sigma_px=inf)]
    for b in bad:
        with pytest.raises(_lib.AslError):
            gpu_detector.locate_tags_device(**{**ok, **b})
    with pytest.raises(ValueError):
        gpu_detector.locate_tags_device(**{**ok, "dist": np.zeros(3)})
    torch.cuda.synchronize()
    assert (d_fit.cpu().numpy() == 0xAB).all() and (d_cov.cpu().numpy() == 0xAB).all()
    assert d_map.cpu().numpy().tobytes() == map_in.tobytes()

    # the host form, through the raw entry point: a NULL K, a bad n_dist, dist NULL with n_dist set
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    Kc = np.ascontiguousarray(K)
    m = map_in.copy()
    fit = np.full(len(m) * 40, 0xAB, dtype=np.uint8)
    args = [gpu_detector._h, obs.ctypes.data, obs.shape[0], obs.shape[1], poses.ctypes.data, m.ctypes.data, len(m), Kc.ctypes.data_as(dp), None, 0,
            QC.TAG, 0.0, 2, 0.0, fit.ctypes.data, None]
    for k, v in ((1, None), (4, None), (5, None), (7, None), (14, None), (9, 3), (9, 4), (3, 300), (6, -2), (2, -1), (12, 0), (11, -1.0), (13, -1.0)):
        a = list(args)
        a[k] = v
        assert L.asl_locate_tags_batch(*a) == -1, (k, v)
        assert (fit == 0xAB).all() and m.tobytes() == map_in.tobytes(), (k, v)
    assert L.asl_locate_tags_batch(*args) == 0                                # cov NULL is not refused
    assert not (fit == 0xAB).all()
    # no frame at all is not an error: every wanted id has too few views
    m0, fit0, cov0 = gpu_detector.locate_tags(obs[:0], poses[:0], map_in, K, None, QC.TAG, sigma_px=0.0)
    odd = QC.odd_ids()
    assert (fit0["status"][odd] == 2).all() and (fit0["n_views"] == 0).all() and m0.tobytes() == map_in.tobytes() and (cov0["status"] == 1).all()
