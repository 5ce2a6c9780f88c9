"""Robust tag-map reconstruction on the device (asl_map_robust_frames_device / asl_map_robust_batch, k_map.inc) against the
NumPy statement (tests/map_ref.py): every field on the repair cases and the small and edge shapes, in the host and
the device form; huber_px 0 through the new entry points against the plain ones, byte for byte; determinism; the repair
against the truth; refusals; TagDetector.build_map(huber_px=)."""
import ctypes as C
import functools

import numpy as np
import pytest

import localize_cases as LC
import map_cases as MC
import map_ref as MR
import map_robust_cases as RC
from aprilslam_amd import _lib, synth
from aprilslam_amd.mapping import MapResult

pytestmark = pytest.mark.gpu

K = RC.K
COMPARED = {c[0]: c[1:] for c in RC.compared_cases()}
INTS = ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft")


@functools.lru_cache(maxsize=None)
def statement(name, iters):
    obs, dist, _ = COMPARED[name]
    return RC.run(obs, dist, max_iters=iters)


def host_form(det, obs, dist, huber=RC.HUBER, iters=RC.ITERS, with_std=True, world_id=-1):
    return det.build_map(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=world_id, max_iters=iters, with_std=with_std, huber_px=huber,
                         with_slot_weight=True)


def device_form(det, obs, dist, huber=RC.HUBER, iters=RC.ITERS, robust=True, fill=None):
    """asl_map_robust_frames_device (robust) or asl_map_frames_device on device buffers; fill: the byte they hold before"""
    import torch
    dev = torch.device("cuda:0")
    n, mt = obs.shape
    u8 = dict(dtype=torch.uint8, device=dev)
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(n, -1)).to(dev)
    bufs = [torch.empty((64,), **u8), torch.empty((MC.N_IDS * _lib.MAP_TAG_DTYPE.itemsize,), **u8), torch.empty((MC.N_IDS * 48,), **u8),
            torch.empty((n * _lib.CAM_POSE_DTYPE.itemsize,), **u8), torch.empty((n * mt * 8,), **u8)]
    for b in bufs:
        b.fill_(0 if fill is None else fill)
    d_res, d_map, d_std, d_poses, d_w = bufs
    kw = dict(huber_px=huber, slot_weight_ptr=d_w.data_ptr()) if robust else {}
    try:
        det.build_map_device(d_obs.data_ptr(), n, mt, MC.N_IDS, K, dist, LC.TAG_INNER, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                             d_res.data_ptr(), max_iters=iters, **kw)
        failed = None
    except _lib.AslError as e:
        failed = e
    torch.cuda.synchronize(dev)
    raw = [b.cpu().numpy() for b in bufs]
    if fill is not None:
        return failed, raw
    assert failed is None, failed
    return (raw[0].view(_lib.MAP_RESULT_DTYPE).reshape(()), raw[1].view(_lib.MAP_TAG_DTYPE).reshape(MC.N_IDS), raw[2].view(np.float64).reshape(-1, 6),
            raw[3].view(_lib.CAM_POSE_DTYPE).reshape(n), raw[4].view(np.float64).reshape(n, mt))


def assert_fields(got, want, tol, what):
    gr, gm, gs, gp, gw = got
    wr, wm, ws, wp, ww = want
    for k in INTS:
        assert gr[k] == wr[k], (what, k, int(gr[k]), int(wr[k]))
    for k in ("cost", "rms_px"):
        assert abs(gr[k] - wr[k]) <= max(tol, 1e-9) * max(1.0, abs(wr[k])), (what, k, float(gr[k]), float(wr[k]))
    for k in ("cost_seed", "rms_seed_px"):      # the seed is the plain call's: test_gpu_map.py's bound for its figures
        assert abs(gr[k] - wr[k]) <= 1e-6 * max(1.0, abs(wr[k])), (what, k, float(gr[k]), float(wr[k]))
    assert np.array_equal(gm["valid"], wm["valid"]), what
    assert RC.distance(got, want) <= tol, (what, RC.distance(got, want))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(gp[k], wp[k]), (what, k)
    used = wp["status"] == 0
    # the per-frame figures at test_gpu_map.py's bound for them: a frame's seed residual carries the flip test's polish
    np.testing.assert_allclose(gp["rms_px"][used], wp["rms_px"][used], rtol=1e-6, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(gp["rms_seed_px"][used], wp["rms_seed_px"][used], rtol=1e-6, atol=1e-6, err_msg=what)
    assert np.array_equal(gw == 0, ww == 0) and np.array_equal(gw < 1, ww < 1), what
    assert np.abs(gw - ww).max() <= max(tol, 1e-9), (what, np.abs(gw - ww).max())
    # the std goes through the inverse of the reduced system: test_gpu_map.py's bound for it
    np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-12, err_msg=what)


@pytest.mark.parametrize("case", sorted(COMPARED))
def test_device_matches_the_statement(gpu_detector, case):
    """both forms, every field; a case whose trial count its tail's rounding decides is compared at COMPARE_ITERS trials,
    and its converged result within ten times the statement's own perturbed distance"""
    obs, dist, iters = COMPARED[case]
    want = statement(case, iters)
    host = host_form(gpu_detector, obs, dist, iters=iters)
    dev = device_form(gpu_detector, obs, dist, iters=iters)
    print(case, "trials", int(host[0]["iterations"]), "n_soft", int(host[0]["n_soft"]), "distance %.3g" % RC.distance(host, want))
    assert_fields(host, want, RC.DEVICE_TOL, case + " host form")
    assert_fields(dev, want, RC.DEVICE_TOL, case + " device form")
    assert all(h.tobytes() == d.tobytes() for h, d in zip(host, dev)), case
    if case in RC.TAIL_CASES:
        conv, wconv = host_form(gpu_detector, obs, dist), statement(case, RC.ITERS)
        d = RC.distance(conv, wconv)
        print(case, "converged: trials %d / %d distance %.3g" % (conv[0]["iterations"], wconv[0]["iterations"], d))
        assert conv[0]["status"] == 0 and conv[0]["iterations"] < RC.ITERS
        assert d <= 10 * RC.TAIL_CASES[case], (case, d)


def test_an_observation_behind_the_camera_has_weight_0(gpu_detector):
    obs, dist, _ = COMPARED["behind"]
    res, tmap, _, poses, w = host_form(gpu_detector, obs, dist)
    assert res["status"] == 0 and res["n_obs_dropped"] == 1 and poses["n_rejected"][0] == 1
    assert w[0, 7] == 0.0 and obs["id"][0, 7] == 7 and not tmap["valid"][7] and (w[obs["id"] >= 0] > 0).sum() == res["n_obs"]


@pytest.mark.parametrize("case", [c[0] for c in MC.cpu_cases(K)])
def test_huber_0_is_the_plain_call_byte_for_byte(gpu_detector, case):
    name, obs, dist, w = [c for c in MC.cpu_cases(K) if c[0] == case][0]
    for with_std in (True, False):
        plain = gpu_detector.build_map(obs, MC.N_IDS, K, dist, LC.TAG_INNER, world_id=w, with_std=with_std)
        got = host_form(gpu_detector, obs, dist, huber=0.0, iters=30, with_std=with_std, world_id=w)
        assert all((g is None and p is None) or g.tobytes() == p.tobytes() for g, p in zip(got[:4], plain)), (case, with_std)
        assert got[0]["n_soft"] == 0
        weight = got[4]
        assert set(np.unique(weight)) <= {0.0, 1.0} and weight.sum() == (plain[0]["n_obs"] if plain[0]["status"] == 0 else 0)
        assert not weight[obs["id"] < 0].any()
    if w == -1:
        a = device_form(gpu_detector, obs, dist, huber=0.0, iters=30)
        b = device_form(gpu_detector, obs, dist, iters=30, robust=False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])), case
        assert np.array_equal(a[4], weight)


def test_without_the_slot_weights_nothing_else_changes(gpu_detector):
    obs, _, _, dist, _ = RC.repair_cases()["small_swap"]
    a = host_form(gpu_detector, obs, dist)
    b = gpu_detector.build_map(obs, MC.N_IDS, K, dist, LC.TAG_INNER, max_iters=RC.ITERS, huber_px=RC.HUBER)
    assert len(b) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b))
    c = gpu_detector.build_map(obs, MC.N_IDS, K, dist, LC.TAG_INNER, max_iters=RC.ITERS, huber_px=RC.HUBER, with_std=False)
    assert c[2] is None and all(x.tobytes() == y.tobytes() for x, y in zip((a[0], a[1], a[3]), (c[0], c[1], c[3])))


def test_the_same_robust_input_gives_the_same_bytes(gpu_detector):
    obs, _, _, dist, _ = RC.repair_cases()["dist5_swap"]
    a = host_form(gpu_detector, obs, dist)
    b = host_form(gpu_detector, obs, dist)
    assert a[0]["n_soft"] >= 1 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = host_form(gpu_detector, np.concatenate([obs, RC.empty_frames(5, obs.shape[1])]), dist)
    assert a[1].tobytes() == c[1].tobytes() and a[2].tobytes() == c[2].tobytes() and a[3].tobytes() == c[3][:12].tobytes()
    assert a[4].tobytes() == c[4][:12].tobytes() and not c[4][12:].any()


@pytest.mark.parametrize("case", sorted(RC.ROBUST_MEASURED))
def test_repair_on_the_device_stays_under_the_recorded_bars(gpu_detector, case):
    obs, tags, cams, dist, bad = RC.repair_cases()[case]
    out = host_form(gpu_detector, obs, dist)
    e = MC.map_errors(out[1], out[3], tags, cams, int(out[0]["world_id"]))
    print(case, "device errors %.4g %.4g %.4g" % e, "trials", int(out[0]["iterations"]), "n_soft", int(out[0]["n_soft"]))
    assert out[0]["status"] == 0
    assert all(g <= 2 * r for g, r in zip(e, RC.ROBUST_MEASURED[case])), (case, e)
    # the corrupted slots exactly; the slip in a seed slot also softens one more slot of its frame (map_robust_cases.EXTRA_SOFT)
    soft = [(f, s) for f, s, _, _ in MapResult(*out[:4], slot_weight=out[4], slot_ids=obs["id"]).soft_slots()]
    assert soft == sorted(bad + RC.EXTRA_SOFT.get(case, [])) and out[0]["n_soft"] == len(soft), (case, soft)


def test_bad_thresholds_are_refused_and_nothing_is_written(gpu_detector):
    obs = np.ascontiguousarray(RC.repair_cases()["small_slip"][0])
    n, mt = obs.shape
    L, h = gpu_detector._L, gpu_detector._h
    Kc = np.ascontiguousarray(K)
    for bad in (-1.0, float("nan"), float("inf")):
        outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (MC.N_IDS * 104, MC.N_IDS * 48, n * 160, 64, n * mt * 8)]
        rc = L.asl_map_robust_batch(h, obs.ctypes.data, n, mt, MC.N_IDS, Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, LC.TAG_INNER, -1,
                                    bad, 30, *[o.ctypes.data for o in outs])
        assert rc == -1 and b"huber_px" in L.asl_last_error(), bad
        assert all((o == 0xAB).all() for o in outs), bad
        failed, raw = device_form(gpu_detector, obs, None, huber=bad, fill=0xCD)
        assert failed is not None and "huber_px" in str(failed), bad
        assert all((r == 0xCD).all() for r in raw), bad
    outs = [np.full(k, 0xAB, dtype=np.uint8) for k in (MC.N_IDS * 104, MC.N_IDS * 48, n * 160, 64, n * mt * 8)]
    assert L.asl_map_robust_batch(h, obs.ctypes.data, n, 257, MC.N_IDS, Kc.ctypes.data_as(C.POINTER(C.c_double)), None, 0, LC.TAG_INNER, -1,
                                  RC.HUBER, 30, *[o.ctypes.data for o in outs]) == -1
    assert all((o == 0xAB).all() for o in outs)


def test_tag_detector_build_map_with_a_threshold():
    import torch

    import bench
    from aprilslam_amd.tag_detector import TagDetector
    dev = torch.device("cuda:0")
    n = 8
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        frames, _, _ = bench.render_stream_device(det, n, dev)
        host = frames.cpu().numpy()
    finally:
        det.close()
    Kr = synth.camera_matrix(LC.W, LC.H, 45.0)
    td = TagDetector({"camera_matrix": Kr, "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER)
    plain = td.build_map(list(host))
    m = td.build_map(list(host), huber_px=1.0)
    assert plain.ok and m.ok and plain.n_soft == 0 and plain.slot_weight is None
    assert m.n_soft == 0 and m.soft_slots() == [] and m.slot_weight.shape == m.slot_ids.shape
    assert (m.slot_weight == 1.0).sum() == int(m.result["n_obs"])
    assert np.array_equal(m.records["valid"], plain.records["valid"])
    for i in np.flatnonzero(m.records["valid"]):
        assert LC.rel_err(MR.rec4(m.records["T"][i]), MR.rec4(plain.records["T"][i])) <= 1e-9, i
