"""Tag-map reconstruction for tags of different known sizes on the device (asl_map_sized_* / asl_map_rig_sized_*, k_map.inc)
against the NumPy statement (tests/map_ref.py): the truth on exact data, every field of the host and device forms on
the cases of tests/map_sized_cases.py (tests/test_map_sized_ref.py checks on the CPU what each is for), the bytes of the
existing calls, refusals, the round trip through the localisation, and TagDetector.build_map(tag_sizes=)."""
import ctypes as C
import functools

import numpy as np
import pytest

import localize_cases as LC
import map_ref as MR
import map_sized_cases as ZC
import sized_cases as SC
from aprilslam_amd import _lib, synth
from test_gpu_map_rig import assert_fields

pytestmark = pytest.mark.gpu

COMPARED = {(c[0], c[4]): (c[1], c[2], c[3], c[5]) for c in ZC.compared_cases()}
IDS = ["%s-huber%g" % k for k in sorted(COMPARED)]
FP = C.POINTER(C.c_float)


@functools.lru_cache(maxsize=None)
def statement(name, huber, iters):
    obs, rig, t, _ = COMPARED[(name, huber)]
    return ZC.run(obs, rig, t, huber, iters)


def single(rig):
    return len(rig.cameras) == 1


def host_form(det, obs, rig, t, huber=0.0, iters=ZC.ITERS, n_ids=ZC.N_IDS, tag=ZC.TAG):
    """the five outputs, slot weights (n_cams, n_frames, max_tags); one camera: asl_map_sized_batch on its stream, else the rig
    form.  t None: the existing robust / rig call"""
    if single(rig):
        cam = rig.cameras[0]
        out = det.build_map(obs[0], n_ids, cam.K, cam.dist if len(cam.dist) else None, tag, max_iters=iters, huber_px=huber, with_slot_weight=True,
                            tag_sizes=t)
        return out[:4] + (out[4][None],)
    return det.build_map_rig(obs, n_ids, rig, tag, max_iters=iters, huber_px=huber, with_slot_weight=True, tag_sizes=t)


def device_form(det, obs, rig, t, huber=0.0, iters=ZC.ITERS, fill=None, n_ids=ZC.N_IDS):
    """the device entry points on device buffers; fill: the byte the outputs hold before (then (error, raw bytes))"""
    import torch
    dev = torch.device("cuda:0")
    nc, n, mt = obs.shape
    u8 = dict(dtype=torch.uint8, device=dev)
    d_obs = torch.from_numpy(np.ascontiguousarray(obs).view(np.uint8).reshape(nc * n, -1)).to(dev)
    d_rig = torch.from_numpy(np.ascontiguousarray(rig.as_records()).view(np.uint8)).to(dev)
    bufs = [torch.empty((64,), **u8), torch.empty((n_ids * _lib.MAP_TAG_DTYPE.itemsize,), **u8), torch.empty((n_ids * 48,), **u8),
            torch.empty((n * _lib.CAM_POSE_DTYPE.itemsize,), **u8), torch.empty((nc * n * mt * 8,), **u8)]
    for b in bufs:
        b.fill_(0 if fill is None else fill)
    d_res, d_map, d_std, d_poses, d_w = bufs
    try:
        if single(rig):
            cam = rig.cameras[0]
            det.build_map_device(d_obs.data_ptr(), n, mt, n_ids, cam.K, cam.dist if len(cam.dist) else None, ZC.TAG, d_map.data_ptr(), d_std.data_ptr(),
                                 d_poses.data_ptr(), d_res.data_ptr(), max_iters=iters, huber_px=huber, slot_weight_ptr=d_w.data_ptr(), tag_sizes=t)
        else:
            det.build_map_rig_device(d_obs.data_ptr(), nc, n, mt, n_ids, d_rig.data_ptr(), ZC.TAG, d_map.data_ptr(), d_std.data_ptr(), d_poses.data_ptr(),
                                     d_res.data_ptr(), max_iters=iters, huber_px=huber, slot_weight_ptr=d_w.data_ptr(), tag_sizes=t)
        failed = None
    except _lib.AslError as e:
        failed = e
    torch.cuda.synchronize(dev)
    raw = [b.cpu().numpy() for b in bufs]
    if fill is not None:
        return failed, raw
    assert failed is None, failed
    return (raw[0].view(_lib.MAP_RESULT_DTYPE).reshape(()), raw[1].view(_lib.MAP_TAG_DTYPE).reshape(n_ids), raw[2].view(np.float64).reshape(-1, 6),
            raw[3].view(_lib.CAM_POSE_DTYPE).reshape(n), raw[4].view(np.float64).reshape(nc, n, mt))


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_truth(gpu_detector):
    """6 tags, id 5 of side 2 TAG, 6 frames x 4 slots, exact corners and records: the map and the poses are the truth in the
    world tag's gauge within ten times the statement's error on the equal-size scene; the same block through the plain call
    is wrong by the factor the statement measures (0.566: tag 5 at 85 units where it is 95 away), at least a tenth of it"""
    obs, t, gt, gp = ZC.truth_case()
    base, bar = ZC.truth_bar()
    cam = SC.one_camera()
    out = host_form(gpu_detector, obs, cam, t, n_ids=6)
    plain = host_form(gpu_detector, obs, cam, None, n_ids=6)
    e, ep = ZC.truth_err(out, gt, gp), ZC.truth_err(plain, gt, gp)
    print("truth: sized %.3g (statement %.3g, bar %.3g), plain call %.3g (statement %.3g)" % (e, ZC.TRUTH_ERRORS["sized"], bar, ep, ZC.TRUTH_ERRORS["plain"]))
    assert out[0]["status"] == 0 and out[0]["n_tags"] == 6 and (out[3]["status"] == 0).all()
    assert np.array_equal(out[1]["size"], t) and not plain[1]["size"].any()
    assert e <= bar, (e, bar)
    assert ep >= 0.1 * ZC.TRUTH_ERRORS["plain"], ep


@pytest.mark.parametrize("case", sorted(COMPARED), ids=IDS)
def test_device_matches_the_statement(gpu_detector, case):
    """both forms, every field, the size field, and the same bytes from both; a case whose trial count its tail's rounding
    decides is compared at COMPARE_ITERS trials, and its converged result within ten times the statement's own perturbed
    distance"""
    name, huber = case
    obs, rig, t, iters = COMPARED[case]
    want = statement(name, huber, iters)
    host = host_form(gpu_detector, obs, rig, t, huber, iters)
    dev = device_form(gpu_detector, obs, rig, t, huber, iters)
    print(name, huber, "trials", int(host[0]["iterations"]), "views", int(host[0]["n_obs"]), "n_soft", int(host[0]["n_soft"]),
          "distance %.3g" % ZC.distance(host, want))
    assert_fields(host, want, ZC.DEVICE_TOL, "%s %g host form" % case)
    assert_fields(dev, want, ZC.DEVICE_TOL, "%s %g device form" % case)
    assert np.array_equal(host[1]["size"], want[1]["size"]) and np.array_equal(host[1]["size"], np.where(host[1]["valid"], t, 0))
    assert same_bytes(host, dev), case
    if case in ZC.TAIL_CASES:
        conv, wconv = host_form(gpu_detector, obs, rig, t, huber), statement(name, huber, ZC.ITERS)
        d = ZC.distance(conv, wconv)
        print(name, huber, "converged: trials %d / %d distance %.3g" % (conv[0]["iterations"], wconv[0]["iterations"], d))
        assert conv[0]["status"] == 0 and conv[0]["iterations"] < ZC.ITERS
        assert d <= 10 * ZC.TAIL_CASES[case], (case, d)


@pytest.mark.parametrize("name", ["single_mixed", "pair_mixed"])
def test_no_table_and_a_zero_table_are_the_existing_call(gpu_detector, name):
    """NULL and all-zero tables: every output of the matching existing call byte for byte (one camera: the plain and the
    robust call; the rig); every entry an exactly representable tag_size: the same bytes but for map.size; twice the same"""
    obs, rig, t = ZC.main_cases()[name]
    zero = np.zeros(ZC.N_IDS, dtype=np.float32)
    for huber in (0.0, ZC.HUBER):
        old = host_form(gpu_detector, obs, rig, None, huber, 20)
        assert same_bytes(host_form(gpu_detector, obs, rig, zero, huber, 20), old), (name, huber)
        assert same_bytes(device_form(gpu_detector, obs, rig, zero, huber, 20), old), (name, huber)
        same = host_form(gpu_detector, obs, rig, np.full(ZC.N_IDS, ZC.TAG, dtype=np.float32), huber, 20)
        assert same_bytes((same[0], same[2], same[3], same[4]), (old[0], old[2], old[3], old[4])) and same[1]["T"].tobytes() == old[1]["T"].tobytes()
        assert np.array_equal(same[1]["valid"], old[1]["valid"]) and np.array_equal(same[1]["size"], np.where(old[1]["valid"], np.float32(ZC.TAG), 0))
        assert not old[1]["size"].any()
    if single(rig):      # the plain entry point (no threshold, no slot weights) and the sized one called with NULL
        cam = rig.cameras[0]
        plain = gpu_detector.build_map(obs[0], ZC.N_IDS, cam.K, None, ZC.TAG, max_iters=20)
        L, o = _lib.load(), np.ascontiguousarray(obs[0])
        keep, Kp, dpp, nd = _lib._camera(cam.K, None, square=True)
        res, tmap = np.zeros((), dtype=_lib.MAP_RESULT_DTYPE), np.zeros(ZC.N_IDS, dtype=_lib.MAP_TAG_DTYPE)
        std, poses = np.zeros((ZC.N_IDS, 6)), np.zeros(o.shape[0], dtype=_lib.CAM_POSE_DTYPE)
        assert L.asl_map_sized_batch(gpu_detector._h, o.ctypes.data, o.shape[0], o.shape[1], ZC.N_IDS, Kp, dpp, nd, ZC.TAG, None, -1, 0.0, 20,
                                     tmap.ctypes.data, std.ctypes.data, poses.ctypes.data, res.ctypes.data, None) == 0
        assert same_bytes((res, tmap, std, poses), plain)
    a, b = host_form(gpu_detector, obs, rig, t, ZC.HUBER, 20), host_form(gpu_detector, obs, rig, t, ZC.HUBER, 20)
    assert same_bytes(a, b) and not same_bytes(a[:1], host_form(gpu_detector, obs, rig, None, ZC.HUBER, 20)[:1])


@pytest.mark.parametrize("name", ["slots_1x17", "behind"])
def test_refusals_leave_the_outputs_untouched(gpu_detector, name):
    """a size of -1, NaN or +inf: ASL_EINVAL naming the id, sentinel-filled outputs untouched, device and host forms"""
    obs, rig, t = ZC.edge_cases()[name]
    L, h = _lib.load(), gpu_detector._h
    nc, n, mt = obs.shape
    o = np.ascontiguousarray(obs)
    out = [np.full(ZC.N_IDS * 104, 0xAB, np.uint8), np.full(ZC.N_IDS * 48, 0xAB, np.uint8), np.full(n * 160, 0xAB, np.uint8), np.full(64, 0xAB, np.uint8),
           np.full(nc * n * mt * 8, 0xAB, np.uint8)]
    ptrs = [x.ctypes.data for x in out]
    for bad, at in ((-1.0, 0), (np.nan, 5), (np.inf, ZC.N_IDS - 1)):
        tt = t.copy()
        tt[at] = bad
        failed, raw = device_form(gpu_detector, obs, rig, tt, fill=0xAB)
        assert failed is not None and ("tag_sizes[%d]" % at) in str(failed), (bad, failed)
        assert all((r == 0xAB).all() for r in raw), bad
        if single(rig):
            cam = rig.cameras[0]
            keep, Kp, dpp, nd = _lib._camera(cam.K, None, square=True)
            rc = L.asl_map_sized_batch(h, o[0].ctypes.data, n, mt, ZC.N_IDS, Kp, dpp, nd, ZC.TAG, tt.ctypes.data_as(FP), -1, 0.0, 30, *ptrs)
        else:
            rec = rig.as_records()
            rc = L.asl_map_rig_sized_batch(h, o.ctypes.data, nc, n, mt, ZC.N_IDS, rec.ctypes.data, ZC.TAG, tt.ctypes.data_as(FP), -1, 0.0, 30, *ptrs)
        assert rc == -1 and ("tag_sizes[%d]" % at).encode() in L.asl_last_error(), bad
        assert all((x == 0xAB).all() for x in out), bad


def test_the_map_goes_to_the_localisation_as_it_is(gpu_detector):
    """the sized call's map block, unchanged, to localize on the same block: the map solve's frame poses within the truth's bar"""
    obs, t, gt, gp = ZC.truth_case()
    _, bar = ZC.truth_bar()
    cam = SC.one_camera().cameras[0]
    out = host_form(gpu_detector, obs, SC.one_camera(), t, n_ids=6)
    loc = gpu_detector.localize(obs[0], out[1], cam.K, None, ZC.TAG)
    assert (loc["status"] == 0).all()
    d = max(LC.rel_err(a, b) for a, b in zip(loc["T"], out[3]["T"]))
    print("localize against the sized map: largest relative pose difference %.3g (bar %.3g)" % (d, bar))
    assert d <= bar
    unsized = out[1].copy()
    unsized["size"] = 0
    off = gpu_detector.localize(obs[0], unsized, cam.K, None, ZC.TAG)
    assert max(LC.rel_err(a, b) for a, b in zip(off["T"], out[3]["T"])) > 100 * bar       # the sizes are what makes it fit


def test_rig_build_map_carries_the_sizes(gpu_detector):
    obs, rig, t = ZC.edge_cases()["all_sized"]
    m = rig.build_map_sized(gpu_detector, obs, ZC.N_IDS, ZC.TAG, {int(i): float(t[i]) for i in np.flatnonzero(t)}, max_iters=ZC.ITERS)
    raw = host_form(gpu_detector, obs, rig, t)
    assert m.ok and same_bytes((m.result, m.records, m.std, m.poses), raw[:4])
    assert all(m.tag_map.size(i) == t[i] for i in m.tag_map.ids())
    loc = rig.localize(gpu_detector, obs, m.tag_map, ZC.TAG)
    assert (loc["status"] == 0).all() and max(LC.rel_err(a, b) for a, b in zip(loc["T"], m.camera_poses)) <= 1e-5


def test_tag_detector_build_map_with_sizes():
    """rendered bench frames (every tag of one side): stating another side for one id moves that tag and nothing is lost on
    the way from TagDetector.build_map to the kernels; the result's tag_map carries the size"""
    import torch

    import bench
    from aprilslam_amd.tag_detector import TagDetector
    dev = torch.device("cuda:0")
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        frames, _, _ = bench.render_stream_device(det, 8, dev)
        host = frames.cpu().numpy()
    finally:
        det.close()
    Kr = synth.camera_matrix(LC.W, LC.H, 45.0)
    td = TagDetector({"camera_matrix": Kr, "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER)
    plain = td.build_map(list(host))
    k = [i for i in plain.tag_map.ids() if i != plain.world_id][0]
    sized = td.build_map(list(host), tag_sizes={k: 2 * LC.TAG_INNER})
    assert plain.ok and sized.ok and sized.tag_map.size(k) == 2 * LC.TAG_INNER and plain.tag_map.size(k) == 0
    assert np.array_equal(sized.records["valid"], plain.records["valid"])
    moved = LC.rel_err(MR.rec4(sized.records["T"][k]), MR.rec4(plain.records["T"][k]))
    print("tag %d stated at twice the side: relative pose change %.3g" % (k, moved))
    assert moved > 1e-2
    table = np.zeros(int(plain.records.shape[0]) + 3, dtype=np.float32)
    table[k] = 2 * LC.TAG_INNER
    again = td.build_map(list(host), tag_sizes=table)
    assert again.records.tobytes() == sized.records.tobytes()
