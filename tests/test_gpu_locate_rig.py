"""Rig tag location on the device (asl_locate_tags_rig_frames_device / asl_locate_tags_rig_batch, LocateRig of k_locate.inc)
against the NumPy statement (tests/locate_rig_ref.py) on every case of tests/locate_rig_cases.py, against the single-camera
kernel it reduces to, and as one device chain on two rendered cameras: localise the rig against half the map, locate the
other half, localise again against the extended map."""
import functools

import numpy as np
import pytest

import localize_cases as LC
import locate_cases as QC
import locate_rig_cases as ZC
import locate_rig_ref as ZR
import rig_cases as RC
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, POSE_COV_DTYPE, TagMap
from aprilslam_amd.rig import Rig, RigCamera
from solver_checks import dev_bytes

pytestmark = pytest.mark.gpu

T_TOL = 1e-9   # relative, every case (test_gpu_locate's)
ONE_CAMERA = ("exact", "wanted", "gate_cap", "frames_edge_130", "dist5")


@functools.lru_cache(maxsize=None)
def statement(name):
    c = ZC.case(name)
    traces = {}
    out = ZR.locate_tags_rig(c["obs"], c["poses"], c["map_in"], c["rig"], ZC.TAG, c["gate"], c["min_views"], sigma_px=0.0, traces=traces)
    return out, traces


def assert_same(name, got, want, traces, map_in, tol):
    """test_gpu_locate.assert_same's rules: discrete fields equal, T within tol relative, rms and covariance within 1e-6, a
    differing seed_frame only at an equal score; -> the worst T error"""
    (gm, gf, gc), (wm, wf, wc) = got, want
    worst = 0.0
    for i in range(len(wf)):
        g, w = gf[i], wf[i]
        for k in ("status", "n_views", "n_rejected", "seed_mirrored", "reserved"):
            assert g[k] == w[k], (name, i, k, g[k], w[k])
        assert gc["status"][i] == wc["status"][i] and gc["dof"][i] == wc["dof"][i], (name, i)
        if w["status"] != 0:
            assert g["seed_frame"] == -1 and g["rms_px"] == 0 and g["rms_seed_px"] == 0
            assert gm[i].tobytes() == map_in[i].tobytes(), (name, i)          # not located: the entry keeps its bytes
            assert not gc["cov"][i].any()
            continue
        if g["seed_frame"] != w["seed_frame"]:                               # a candidate of equal score
            tv, trace = traces[i][0], traces[i][1]
            sc = {}
            for v, m, c in trace["first"]:                                   # a frame has a candidate per camera: the best of them
                key = (tv.views[v][0], m)
                sc[key] = min(sc.get(key, np.inf), c)
            a, b = sc[(int(g["seed_frame"]), int(g["seed_mirrored"]))], sc[(int(w["seed_frame"]), int(w["seed_mirrored"]))]
            assert abs(a - b) <= 1e-9 * max(1.0, b), (name, i, g["seed_frame"], w["seed_frame"])
        err = LC.rel_err(gm["T"][i], wm["T"][i])
        worst = max(worst, err)
        assert err <= tol, (name, i, err)
        assert gm["valid"][i] == 1 and gm["size"][i].tobytes() == map_in["size"][i].tobytes()
        assert abs(g["rms_px"] - w["rms_px"]) <= 1e-6 * max(1.0, w["rms_px"]), (name, i)
        assert abs(g["rms_seed_px"] - w["rms_seed_px"]) <= 1e-6 * max(1.0, w["rms_seed_px"]), (name, i)
        assert np.array_equal(gc["cov"][i], gc["cov"][i].T)
        if wc["status"][i] == 0:
            assert np.abs(gc["cov"][i] - wc["cov"][i]).max() <= 1e-6 * np.abs(wc["cov"][i]).max(), (name, i)
            assert abs(gc["sigma_px"][i] - wc["sigma_px"][i]) <= 1e-6 * max(1.0, wc["sigma_px"][i])
    return worst


@pytest.mark.parametrize("name", ZC.CASES)
def test_kernel_matches_the_statement(gpu_detector, name):
    c = ZC.case(name)
    want, traces = statement(name)
    map_in = c["map_in"]
    before = map_in.copy()
    got = gpu_detector.locate_tags_rig(c["obs"], c["poses"], map_in, c["rig"], ZC.TAG, max_view_rms_px=c["gate"], min_views=c["min_views"], sigma_px=0.0)
    assert map_in.tobytes() == before.tobytes()                               # the caller's block is not modified
    worst = assert_same(name, got, want, traces, map_in, T_TOL)
    print("%s: worst T rel err %.3g over %d located" % (name, worst, int((want[1]["status"] == 0).sum())))
    assert (want[1]["status"][list(c["truth"])] == 0).all()
    # the plain call and the covariance call write the same map and fit bytes
    plain = gpu_detector.locate_tags_rig(c["obs"], c["poses"], map_in, c["rig"], ZC.TAG, max_view_rms_px=c["gate"], min_views=c["min_views"])
    assert plain[2] is None and plain[0].tobytes() == got[0].tobytes() and plain[1].tobytes() == got[1].tobytes()
    for i, (f, cam) in c.get("spoiled", {}).items():
        if c["gate"]:
            assert got[1]["n_rejected"][i] == 1 and got[1]["rms_px"][i] < 1e-3, (name, i)         # the intact view of the frame stays


@pytest.mark.parametrize("name", ONE_CAMERA)
def test_one_camera_at_the_identity_is_the_single_camera_kernel(gpu_detector, name):
    _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
    wm, wf, wc = gpu_detector.locate_tags(obs, poses, map_in, QC.K, dist, QC.TAG, max_view_rms_px=gate, min_views=min_views, sigma_px=0.0)
    gm, gf, gc = gpu_detector.locate_tags_rig(obs[None], poses, map_in, ZC.solo(QC.K, dist), QC.TAG, max_view_rms_px=gate, min_views=min_views,
                                              sigma_px=0.0)
    print(name, "map bytes identical:", gm.tobytes() == wm.tobytes(), "fit bytes identical:", gf.tobytes() == wf.tobytes(),
          "covariance bytes identical:", gc.tobytes() == wc.tobytes())
    for k in ("status", "n_views", "n_rejected", "seed_frame", "seed_mirrored", "reserved"):
        assert np.array_equal(gf[k], wf[k]), (name, k)
    assert np.array_equal(gm["valid"], wm["valid"]) and gm["size"].tobytes() == wm["size"].tobytes()
    assert np.array_equal(gc["status"], wc["status"]) and np.array_equal(gc["dof"], wc["dof"])
    assert (wf["status"] == 0).any()
    for i in np.flatnonzero(wf["status"] == 0):
        assert LC.rel_err(gm["T"][i], wm["T"][i]) <= T_TOL, (name, i)
    rest = wf["status"] != 0
    assert gm[rest].tobytes() == wm[rest].tobytes()


def _device_call(det, torch, c, with_cov):
    dev = torch.device("cuda:0")
    obs, map_in = c["obs"], c["map_in"]
    d_obs, d_poses, d_map, d_rig = dev_bytes(obs, dev), dev_bytes(c["poses"], dev), dev_bytes(map_in, dev), dev_bytes(c["rig"].as_records(), dev)
    d_fit = torch.zeros(len(map_in) * _lib.TAG_FIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cov = torch.zeros(len(map_in) * POSE_COV_DTYPE.itemsize, dtype=torch.uint8, device=dev) if with_cov else None
    det.locate_tags_rig_device(d_obs.data_ptr(), obs.shape[0], obs.shape[1], obs.shape[2], d_poses.data_ptr(), d_map.data_ptr(), len(map_in),
                               d_rig.data_ptr(), d_fit.data_ptr(), ZC.TAG, max_view_rms_px=c["gate"], min_views=c["min_views"],
                               stream=torch.cuda.current_stream().cuda_stream, cov_ptr=d_cov.data_ptr() if with_cov else None, sigma_px=0.0)
    torch.cuda.synchronize()
    return d_map.cpu().numpy().tobytes(), d_fit.cpu().numpy().tobytes(), d_cov.cpu().numpy().tobytes() if with_cov else None


def test_host_form_and_device_form_give_identical_bytes(gpu_detector):
    import torch
    c = ZC.case("both_cameras")
    m, fit, cov = gpu_detector.locate_tags_rig(c["obs"], c["poses"], c["map_in"], c["rig"], ZC.TAG, max_view_rms_px=c["gate"],
                                               min_views=c["min_views"], sigma_px=0.0)
    dm, dfit, dcov = _device_call(gpu_detector, torch, c, True)
    assert dm == m.tobytes() and dfit == fit.tobytes() and dcov == cov.tobytes()
    pm, pfit, _ = _device_call(gpu_detector, torch, c, False)
    assert pm == dm and pfit == dfit


def test_ten_repeats_give_identical_bytes(gpu_detector):
    import torch
    c = ZC.case("gate_cap")                                                   # the longest path: re-seeds up to the cap
    first = None
    for _ in range(10):
        got = _device_call(gpu_detector, torch, c, True)                     # the map uploaded afresh
        first = got if first is None else first
        assert got == first


def test_refusals_touch_no_output(gpu_detector):
    import torch
    dev = torch.device("cuda:0")
    c = ZC.case("both_cameras")
    obs, poses, map_in, rig = c["obs"], c["poses"], c["map_in"], c["rig"].as_records()
    nc, n, mt = obs.shape
    d_obs, d_poses, d_map, d_rig = dev_bytes(obs, dev), dev_bytes(poses, dev), dev_bytes(map_in, dev), dev_bytes(rig, dev)
    d_fit = torch.full((len(map_in) * 40,), 0xAB, dtype=torch.uint8, device=dev)
    d_cov = torch.full((len(map_in) * 304,), 0xAB, dtype=torch.uint8, device=dev)
    bad_tables = []
    for field, idx, value in (("E", (1, 0, 0), 1.5), ("n_dist", (1,), 3), ("K", (0, 1, 1), np.nan), ("E", (0, 2, 3), np.inf), ("dist", (1, 2), np.nan)):
        t = rig.copy()
        if field == "dist":
            t["n_dist"][1] = 4
        t[field][idx] = value
        bad_tables.append(t)
    nan, inf = float("nan"), float("inf")
    # whatever asl_locate_tags_* refuses, then the rig's own: the table NULL, n_cams outside [1, 16], more than 256 global
    # slots, 2^31 records (16 x 2^23 x 16; refused before anything is read)
    bad = [dict(obs_ptr=0), dict(poses_ptr=0), dict(map_ptr=0), dict(fit_ptr=0), dict(n_frames=-1), dict(max_tags=0), dict(max_tags=257),
           dict(n_ids=0), dict(tag_size=0.0), dict(tag_size=-1.0), dict(tag_size=nan), dict(max_view_rms_px=-0.5), dict(max_view_rms_px=nan),
           dict(max_view_rms_px=inf), dict(min_views=0), dict(min_views=-3), dict(sigma_px=-1.0), dict(sigma_px=nan), dict(sigma_px=inf),
           dict(rig_ptr=0), dict(n_cams=0), dict(n_cams=-1), dict(n_cams=17), dict(n_cams=2, max_tags=129), dict(n_cams=16, max_tags=17),
           dict(n_cams=16, n_frames=1 << 23, max_tags=16)]

    # the device form
    ok = dict(obs_ptr=d_obs.data_ptr(), n_cams=nc, n_frames=n, max_tags=mt, poses_ptr=d_poses.data_ptr(), map_ptr=d_map.data_ptr(), n_ids=len(map_in),
              rig_ptr=d_rig.data_ptr(), fit_ptr=d_fit.data_ptr(), tag_size=ZC.TAG, max_view_rms_px=0.0, min_views=2, cov_ptr=d_cov.data_ptr(), sigma_px=0.0)
    for b in bad:
        with pytest.raises(_lib.AslError):
            gpu_detector.locate_tags_rig_device(**{**ok, **b})
    for t in bad_tables:
        d_bad = dev_bytes(t, dev)
        with pytest.raises(_lib.AslError):
            gpu_detector.locate_tags_rig_device(**{**ok, "rig_ptr": d_bad.data_ptr()})
    torch.cuda.synchronize()
    assert (d_fit.cpu().numpy() == 0xAB).all() and (d_cov.cpu().numpy() == 0xAB).all()
    assert d_map.cpu().numpy().tobytes() == map_in.tobytes()

    # the host form, through the raw entry point
    L = _lib.load()
    m = map_in.copy()
    fit = np.full(len(m) * 40, 0xAB, dtype=np.uint8)
    cov = np.full(len(m) * 304, 0xAB, dtype=np.uint8)
    names = ["det", "obs_ptr", "n_cams", "n_frames", "max_tags", "poses_ptr", "map_ptr", "n_ids", "rig_ptr", "tag_size", "max_view_rms_px", "min_views",
             "sigma_px", "fit_ptr", "cov_ptr"]
    args = [gpu_detector._h, obs.ctypes.data, nc, n, mt, poses.ctypes.data, m.ctypes.data, len(m), rig.ctypes.data, ZC.TAG, 0.0, 2, 0.0, fit.ctypes.data,
            cov.ctypes.data]
    for b in bad + [dict(rig_ptr=t.ctypes.data) for t in bad_tables]:
        a = list(args)
        for k, v in b.items():
            a[names.index(k)] = (v or None) if k.endswith("_ptr") else v
        assert L.asl_locate_tags_rig_batch(*a) == -1, b
        assert (fit == 0xAB).all() and (cov == 0xAB).all() and m.tobytes() == map_in.tobytes(), b
    a = list(args)
    a[names.index("cov_ptr")] = None
    assert L.asl_locate_tags_rig_batch(*a) == 0                               # cov NULL is not refused
    assert not (fit == 0xAB).all() and (cov == 0xAB).all()
    # no frame at all is not an error: every wanted id has too few views
    m0, fit0, cov0 = gpu_detector.locate_tags_rig(obs[:, :0], poses[:0], map_in, rig, ZC.TAG, sigma_px=0.0)
    odd = QC.odd_ids()
    assert (fit0["status"][odd] == 2).all() and (fit0["n_views"] == 0).all() and m0.tobytes() == map_in.tobytes() and (cov0["status"] == 1).all()


CHAIN_FRAMES, CHAIN_MAX_TAGS = 32, 32


@pytest.fixture(scope="module")
def device_chain():
    """Two cameras on one rig (test_gpu_rig's: camera 0 = the rig frame, camera 1 6 units to its right, turned 8 degrees out
    and 1 down) moved along the bench trajectory through the bench scene, 32 frames each: rendered on the device, detected
    and packed into one block -> the rig localised against the even ids -> the odd ids located -> the rig localised against
    the extended map: one stream, one read-back"""
    import torch

    import bench
    dev = torch.device("cuda:0")
    n, mt = CHAIN_FRAMES, CHAIN_MAX_TAGS
    K = synth.camera_matrix(LC.W, LC.H, 45.0)
    tags = LC.bench_scene()
    full = TagMap.from_scene(tags).as_records()
    rec = full.copy()
    rec[1::2] = np.zeros((), dtype=_lib.MAP_TAG_DTYPE)
    E1 = RC.mounting(8.0, (6.0, 0.5, 0.0), 1.0)
    rig = Rig([RigCamera(K, None, np.eye(4)), RigCamera(K, None, E1)])
    cams0 = bench.camera_trajectory(n)
    truth = [LC.world_from_camera(p, r) for p, r in cams0]
    cams = [cams0, [RC.synth_camera(T @ np.linalg.inv(E1)) for T in truth]]
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    d_tex = torch.from_numpy(tex).to(dev)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_obs = torch.empty((2, n, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_map, d_rig = dev_bytes(rec, dev), dev_bytes(rig.as_records(), dev)
    d_out = torch.empty((2, n, CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_fit = torch.empty((len(rec), _lib.TAG_FIT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    dets, keep = [], []
    torch.cuda.synchronize()
    for c in range(2):
        det = _lib.Detector("tagStandard41h12", id_limit=0)
        planes, _ = synth.render_planes(LC.W, LC.H, tags, LC.TAG_OUTER, cams[c])
        d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
        frames = torch.empty((n, LC.H, LC.W, 3), dtype=torch.uint8, device=dev)
        keep += [d_planes, frames]
        det.render_frames_device(frames.data_ptr(), n, LC.W, LC.H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2],
                                 tex.shape[1], 0.5 * LC.TAG_OUTER, stream=st)
        det.submit_device(frames.data_ptr(), n, 3, LC.W, LC.H, stream=st, K=K, dist=np.zeros(4), tag_size=LC.TAG_INNER)
        det.pack_observations_device(d_obs[c].data_ptr(), mt, stream=st)
        dets.append(det)
    det = dets[0]
    det.localize_rig_device(d_obs.data_ptr(), 2, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_out[0].data_ptr(), LC.TAG_INNER, stream=st)
    det.locate_tags_rig_device(d_obs.data_ptr(), 2, n, mt, d_out[0].data_ptr(), d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_fit.data_ptr(),
                               LC.TAG_INNER, max_view_rms_px=QC.GATE, stream=st)
    det.localize_rig_device(d_obs.data_ptr(), 2, n, mt, d_map.data_ptr(), len(rec), d_rig.data_ptr(), d_out[1].data_ptr(), LC.TAG_INNER, stream=st)
    stream.synchronize()
    out = d_out.cpu().numpy().view(CAM_POSE_DTYPE).reshape(2, n)
    fit = d_fit.cpu().numpy().view(_lib.TAG_FIT_DTYPE).reshape(len(rec))
    ext = d_map.cpu().numpy().view(_lib.MAP_TAG_DTYPE).reshape(len(rec))
    for d in dets:
        d.collect()
    yield rec, full, ext, fit, out[0], out[1], truth
    for d in dets:
        d.close()


def test_device_chain_extends_the_map_and_the_frames_use_it(device_chain):
    rec, full, ext, fit, first, second, truth = device_chain
    odd = np.arange(1, len(rec), 2)
    assert (fit["status"][odd] == 0).all() and (fit["status"][::2] == 1).all()
    assert ext[::2].tobytes() == rec[::2].tobytes() and (ext["valid"] == 1).all()
    assert (first["status"] == 0).all() and (second["status"] == 0).all()
    assert (second["n_tags"] > first["n_tags"]).all()
    for i in odd:
        T = np.vstack([full["T"][i].reshape(3, 4), [0, 0, 0, 1]])
        dp, dr = QC.pose_errors(ext["T"][i], T)
        print("id %d: %d views, %d rejected, rms %.3f px, %.3f units and %.3f mrad from the scene" % (i, fit["n_views"][i], fit["n_rejected"][i], fit["rms_px"][i], dp, dr * 1e3))
        assert fit["rms_px"][i] < 1.0
    for what, p in (("first", first), ("second", second)):
        rot = np.array([LC.rot_err(T, t) for T, t in zip(p["T"], truth)])
        tr = np.array([np.linalg.norm(T[:3, 3] - t[:3, 3]) for T, t in zip(p["T"], truth)]) * LC.MM_PER_UNIT
        print("%s pass, world<-rig against the renderer: %.4f mrad %.4f mm RMS over %d frames" % (what, np.sqrt(np.mean(rot ** 2)) * 1e3, np.sqrt(np.mean(tr ** 2)), len(p)))
