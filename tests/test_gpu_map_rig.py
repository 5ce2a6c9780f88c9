"""Tag-map reconstruction from a camera rig's frames on the device (asl_map_rig_frames_device / asl_map_rig_batch, k_map.inc)
against the NumPy statement (tests/map_ref.py): every field of both entry points on the split, overlap and mixed-model
blocks and the edge shapes, with and without the Huber loss; one camera with E = I against asl_map_robust_frames_device;
determinism; the slot weights; refusals; Rig.build_map and Rig.localize against the map it returns."""
import ctypes as C
import functools

import numpy as np
import pytest

import localize_cases as LC
import map_rig_cases as GC
from aprilslam_amd import _lib
from aprilslam_amd.mapping import MapResult
from aprilslam_amd.rig import Rig, RigCamera

pytestmark = pytest.mark.gpu

COMPARED = {(c[0], c[3]): (c[1], c[2], c[4]) for c in GC.compared_cases()}
INTS = ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft")
IDS = ["%s-huber%g" % k for k in sorted(COMPARED)]


@functools.lru_cache(maxsize=None)
def statement(name, huber, iters):
    obs, rig, _ = COMPARED[(name, huber)]
    return GC.run(obs, rig, huber=huber, max_iters=iters)


def host_form(det, obs, rig, huber=0.0, iters=GC.ITERS, with_std=True, world_id=-1, with_slot_weight=True):
    return det.build_map_rig(obs, GC.N_IDS, rig, GC.TAG, world_id=world_id, max_iters=iters, with_std=with_std, huber_px=huber,
                             with_slot_weight=with_slot_weight)


def device_form(det, obs, rig, huber=0.0, iters=GC.ITERS, fill=None, n_cams=None, rig_null=False, max_tags=None):
    """asl_map_rig_frames_device on device buffers; fill: the byte the outputs hold before (then (error, raw bytes))"""
    import torch
    dev = torch.device("cuda:0")
    nc, n, mt = obs.shape
    u8 = dict(dtype=torch.uint8, device=dev)
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(nc * n, -1)).to(dev)
    rec = rig.as_records() if hasattr(rig, "as_records") else np.asarray(rig, dtype=_lib.RIG_CAMERA_DTYPE)
    d_rig = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8)).to(dev)
    bufs = [torch.empty((64,), **u8), torch.empty((GC.N_IDS * _lib.MAP_TAG_DTYPE.itemsize,), **u8), torch.empty((GC.N_IDS * 48,), **u8),
            torch.empty((n * _lib.CAM_POSE_DTYPE.itemsize,), **u8), torch.empty((nc * n * mt * 8,), **u8)]
    for b in bufs:
        b.fill_(0 if fill is None else fill)
    d_res, d_map, d_std, d_poses, d_w = bufs
    try:
        det.build_map_rig_device(d_obs.data_ptr(), nc if n_cams is None else n_cams, n, mt if max_tags is None else max_tags, GC.N_IDS,
                                 0 if rig_null else d_rig.data_ptr(), GC.TAG, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                                 d_res.data_ptr(), max_iters=iters, huber_px=huber, slot_weight_ptr=d_w.data_ptr())
        failed = None
    except _lib.AslError as e:
        failed = e
    torch.cuda.synchronize(dev)
    raw = [b.cpu().numpy() for b in bufs]
    if fill is not None:
        return failed, raw
    assert failed is None, failed
    return (raw[0].view(_lib.MAP_RESULT_DTYPE).reshape(()), raw[1].view(_lib.MAP_TAG_DTYPE).reshape(GC.N_IDS), raw[2].view(np.float64).reshape(-1, 6),
            raw[3].view(_lib.CAM_POSE_DTYPE).reshape(n), raw[4].view(np.float64).reshape(nc, n, mt))


def assert_fields(got, want, tol, what, ints=INTS):
    """test_gpu_map_robust.py's comparison of every field"""
    gr, gm, gs, gp, gw = got
    wr, wm, ws, wp, ww = want
    for k in ints:
        assert gr[k] == wr[k], (what, k, int(gr[k]), int(wr[k]))
    for k in ("cost", "rms_px"):
        assert abs(gr[k] - wr[k]) <= max(tol, 1e-9) * max(1.0, abs(wr[k])), (what, k, float(gr[k]), float(wr[k]))
    for k in ("cost_seed", "rms_seed_px"):      # the seed carries the flip test's polish: test_gpu_map.py's bound for its figures
        assert abs(gr[k] - wr[k]) <= 1e-6 * max(1.0, abs(wr[k])), (what, k, float(gr[k]), float(wr[k]))
    assert np.array_equal(gm["valid"], wm["valid"]), what
    assert GC.distance(got, want) <= tol, (what, GC.distance(got, want))
    for k in ("status", "n_tags", "n_rejected", "seed_slot"):
        assert np.array_equal(gp[k], wp[k]), (what, k, gp[k], wp[k])
    used = wp["status"] == 0
    np.testing.assert_allclose(gp["rms_px"][used], wp["rms_px"][used], rtol=1e-6, atol=1e-6, err_msg=what)
    np.testing.assert_allclose(gp["rms_seed_px"][used], wp["rms_seed_px"][used], rtol=1e-6, atol=1e-6, err_msg=what)
    if gw is not None:
        assert np.array_equal(gw == 0, ww == 0) and np.array_equal(gw < 1, ww < 1), what
        assert np.abs(gw - ww).max() <= max(tol, 1e-9), (what, np.abs(gw - ww).max())
    # the std goes through the inverse of the reduced system: test_gpu_map.py's bound for it
    np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-12, err_msg=what)


@pytest.mark.parametrize("case", sorted(COMPARED), ids=IDS)
def test_device_matches_the_statement(gpu_detector, case):
    """both forms, every field, and the same bytes from both; a case whose trial count its tail's rounding decides is
    compared at COMPARE_ITERS trials, and its converged result within ten times the statement's own perturbed distance"""
    name, huber = case
    obs, rig, iters = COMPARED[case]
    want = statement(name, huber, iters)
    host = host_form(gpu_detector, obs, rig, huber, iters)
    dev = device_form(gpu_detector, obs, rig, huber, iters)
    print(name, huber, "trials", int(host[0]["iterations"]), "views", int(host[0]["n_obs"]), "n_soft", int(host[0]["n_soft"]),
          "distance %.3g" % GC.distance(host, want))
    assert_fields(host, want, GC.DEVICE_TOL, "%s %g host form" % case)
    assert_fields(dev, want, GC.DEVICE_TOL, "%s %g device form" % case)
    assert all(h.tobytes() == d.tobytes() for h, d in zip(host, dev)), case
    if case in GC.TAIL_CASES:
        conv, wconv = host_form(gpu_detector, obs, rig, huber), statement(name, huber, GC.ITERS)
        d = GC.distance(conv, wconv)
        print(name, huber, "converged: trials %d / %d distance %.3g" % (conv[0]["iterations"], wconv[0]["iterations"], d))
        assert conv[0]["status"] == 0 and conv[0]["iterations"] < GC.ITERS
        assert d <= 10 * GC.TAIL_CASES[case], (case, d)


def test_the_shapes_hold_what_they_are_for():
    """the statement's own look at the edge inputs: the 16-view pair, the lists of 16 and 17 views, the frame left unused,
    the pair whose first view the behind test drops (no device work; here because the device comparison rests on it)"""
    e = GC.edge_cases()
    obs, _ = e["slots_16x16"]
    per_pair = {}
    for c, f, s in np.argwhere(obs["id"] >= 0):
        per_pair[(f, int(obs["id"][c, f, s]))] = per_pair.get((f, int(obs["id"][c, f, s])), 0) + 1
    assert max(per_pair.values()) == 16
    obs, _ = e["list_16_17"]
    assert (obs["id"] == 3).sum() == 16 and (obs["id"] == 4).sum() == 17
    lone = statement("lone_pair_frame", 0.0, GC.ITERS)
    assert lone[3]["status"][GC.LONE_FRAME] == 1 and lone[3]["n_rejected"][GC.LONE_FRAME] == 0 and (np.delete(lone[3]["status"], GC.LONE_FRAME) == 0).all()
    out = statement("behind", 0.0, GC.ITERS)
    assert out[0]["status"] == 0 and out[0]["n_obs_dropped"] == 1 and out[3]["n_rejected"][1] == 1 and out[4][0, 1, 2] == 0.0
    assert out[1]["valid"][2] and out[4][1, 1][e["behind"][0]["id"][1, 1] == 2] == 1.0
    obs, _ = e["disjoint"]
    assert not set(obs["id"][0].ravel()) & set(obs["id"][1].ravel()) - {-1} and GC.view_counts(obs)[0] == GC.view_counts(obs)[1]


def test_one_camera_at_the_identity_is_the_single_camera_solve(gpu_detector):
    """asl_map_robust_frames_device on the same block: integer fields equal, doubles under the device's bound"""
    obs, rig = GC.edge_cases()["slots_1x17"]
    cam = rig.cameras[0]
    for huber in (0.0, GC.HUBER):
        got = host_form(gpu_detector, obs, rig, huber)
        want = gpu_detector.build_map(obs[0], GC.N_IDS, cam.K, None, GC.TAG, max_iters=GC.ITERS, huber_px=huber, with_slot_weight=True)
        want = want[:4] + (want[4][None],)
        assert_fields(got, want, GC.DEVICE_TOL, "one camera, huber %g" % huber)


def test_huber_0_with_and_without_the_slot_weights(gpu_detector):
    obs, rig = GC.main_cases()["overlap"]
    a = host_form(gpu_detector, obs, rig)
    b = host_form(gpu_detector, obs, rig, with_slot_weight=False)
    assert len(b) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b))
    assert a[0]["n_soft"] == 0 and set(np.unique(a[4])) <= {0.0, 1.0} and a[4].sum() == a[0]["n_obs"] and not a[4][obs["id"] < 0].any()
    c = host_form(gpu_detector, obs, rig, with_std=False)
    assert c[2] is None and all(x.tobytes() == y.tobytes() for x, y in zip((a[0], a[1], a[3], a[4]), (c[0], c[1], c[3], c[4])))


def test_the_same_input_gives_the_same_bytes(gpu_detector):
    obs, rig = GC.main_cases()["mixed_models"]
    a = host_form(gpu_detector, obs, rig, GC.HUBER)
    b = host_form(gpu_detector, obs, rig, GC.HUBER)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def bad_table(rig, c, field, value):
    rec = rig.as_records()
    flat = rec[field][c].reshape(-1) if rec[field][c].ndim else None
    if flat is None:
        rec[field][c] = value
    else:
        flat[0] = value
    return rec


def test_refusals_leave_the_outputs_untouched(gpu_detector):
    obs, rig = GC.edge_cases()["disjoint"]
    skew = rig.as_records()
    skew["E"][1][0, 0] += 1e-4
    calls = [dict(rig_null=True), dict(n_cams=0), dict(n_cams=17), dict(max_tags=129), dict(huber=-1.0), dict(huber=float("nan")), dict(iters=0),
             dict(rig=bad_table(rig, 1, "n_dist", 3)), dict(rig=bad_table(rig, 0, "K", np.nan)), dict(rig=bad_table(rig, 1, "E", np.inf)),
             dict(rig=skew)]
    for kw in calls:
        args = dict(rig=rig)
        args.update(kw)
        failed, raw = device_form(gpu_detector, obs, fill=0xAB, **args)
        assert failed is not None, kw
        assert all((r == 0xAB).all() for r in raw), kw
    L, h = _lib.load(), gpu_detector._h
    nc, n, mt = obs.shape
    rec = rig.as_records()
    out = [np.full(64, 0xAB, np.uint8), np.full(GC.N_IDS * 104, 0xAB, np.uint8), np.full(GC.N_IDS * 48, 0xAB, np.uint8),
           np.full(n * 160, 0xAB, np.uint8), np.full(nc * n * mt * 8, 0xAB, np.uint8)]

    def host(n_cams=nc, table=rec, n_ids=GC.N_IDS, world=-1):
        return L.asl_map_rig_batch(h, obs.ctypes.data, n_cams, n, mt, n_ids, table.ctypes.data if table is not None else None, GC.TAG, world, 0.0,
                                   30, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, out[0].ctypes.data, out[4].ctypes.data)

    for kw in (dict(table=None), dict(n_cams=17), dict(n_ids=0), dict(world=GC.N_IDS), dict(table=skew), dict(table=bad_table(rig, 0, "n_dist", 6))):
        assert host(**kw) == -1, kw         # ASL_EINVAL
        assert all((o == 0xAB).all() for o in out), kw


def test_rig_build_map_and_localize_against_it(gpu_detector):
    """Rig.build_map returns the ctypes call's bytes, and Rig.localize against the returned map gives the solve's own rig
    poses to 1e-5 of the tag size"""
    obs, rig = GC.main_cases()["overlap"]
    m = rig.build_map(gpu_detector, obs, GC.N_IDS, GC.TAG, max_iters=GC.ITERS, huber_px=GC.HUBER)
    raw = host_form(gpu_detector, obs, rig, GC.HUBER)
    assert isinstance(m, MapResult) and m.ok and m.world_id == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip((m.result, m.records, m.std, m.poses, m.slot_weight), raw))
    assert m.slot_weight.shape == obs.shape and all(len(t) == 5 for t in m.soft_slots())
    plain = rig.build_map(gpu_detector, obs, GC.N_IDS, GC.TAG, max_iters=GC.ITERS)
    assert plain.slot_weight is None and plain.n_soft == 0
    loc = rig.localize(gpu_detector, obs, plain.tag_map, GC.TAG)
    assert (loc["status"] == 0).all()
    d = np.abs(loc["T"] - plain.camera_poses)[:, :3, 3].max()
    print("localize against the built map: largest translation difference %.3g" % d)
    assert d <= 1e-5 * GC.TAG
    assert max(LC.rel_err(a, b) for a, b in zip(loc["T"], plain.camera_poses)) <= 1e-5
