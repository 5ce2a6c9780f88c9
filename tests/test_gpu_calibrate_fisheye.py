"""Fisheye camera calibration on the device (asl_calibrate_lens_frames_device / asl_calibrate_lens_batch, k_calib.inc)
against the NumPy statement (tests/calib_fisheye_ref.py), the Brown lens through the new entry points against the old
ones, the refusals, and the chain raw fisheye frames -> calibrate -> views -> detector."""
import numpy as np
import pytest

import calib_cases as CC
import calib_fisheye_cases as FC
import calib_fisheye_ref as FR
import localize_cases as LC
from aprilslam_amd import _lib
from aprilslam_amd.calibrate import CALIB_RESULT_DTYPE, CalibrationResult
from aprilslam_amd.localize import CAM_POSE_DTYPE
from test_gpu_calibrate import assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c[0] for c in FC.cases()])
def test_kernel_matches_the_statement(gpu_detector, name):
    _, obs, rec, kw = FC.case(name)
    got = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, model="fisheye", **kw)
    want = FR.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, **kw)
    print(name, got[0]["K"].ravel()[[0, 4, 2, 5]], got[0]["dist"], got[0]["rms_px"], got[0]["rms_init_px"], got[0]["iterations"], want[0]["iterations"])
    assert_same(got, want, 1e-9)
    assert np.array_equal(got[1]["seed_slot"], want[1]["seed_slot"])
    assert got[0]["dist"][4] == 0 and got[0]["std"][8] == 0


def test_device_form_on_one_stream_repeats_its_bytes(gpu_detector):
    import torch
    dev = torch.device("cuda:0")
    _, obs, rec, kw = FC.case("board4")
    want = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, model="fisheye", **kw)
    d_obs = torch.from_numpy(obs.view(np.uint8).copy()).to(dev)
    d_map = torch.from_numpy(rec.view(np.uint8)).to(dev)
    d_res = torch.empty(CALIB_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_poses = torch.empty((len(obs), CAM_POSE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    for _ in range(2):
        with torch.cuda.stream(stream):
            d_res.zero_()
            d_poses.zero_()
        gpu_detector.calibrate_device(d_obs.data_ptr(), len(obs), obs.shape[1], d_map.data_ptr(), len(rec), LC.TAG_INNER, FC.W, FC.H,
                                      d_res.data_ptr(), d_poses.data_ptr(), stream=stream.cuda_stream, model="fisheye", **kw)
        stream.synchronize()
        assert d_res.cpu().numpy().tobytes() == want[0].tobytes()
        assert d_poses.cpu().numpy().tobytes() == want[1].tobytes()


def test_brown_through_the_new_entry_is_the_old_call_byte_for_byte(gpu_detector):
    name, obs, rec, kw = [c for c in CC.cpu_cases() if c[0] == "scene5"][0]
    old = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, **kw)
    new = gpu_detector.calibrate(obs, rec, LC.TAG_INNER, CC.W, CC.H, model="brown", **kw)
    assert old[0]["status"] == 0
    assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes()


def test_argument_errors(gpu_detector):
    _, obs, rec, _ = FC.case("board4")
    L = _lib.load()
    res = np.full(216, 0xAB, dtype=np.uint8)
    poses = np.full(len(obs) * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    # detector, obs, n_frames, max_tags, map, n_ids, tag_size, width, height, K_init, lens_model, n_dist, flags, max_iters, result, poses
    args = [gpu_detector._h, obs.ctypes.data, len(obs), obs.shape[1], rec.ctypes.data, len(rec), LC.TAG_INNER, FC.W, FC.H, None, 1, 4, 0, 2,
            res.ctypes.data, poses.ctypes.data]
    bad = [(10, 2), (10, -1), (11, 5), (11, 3), (12, 4), (12, 8),                      # the lens, its coefficients, its flags
           (1, None), (4, None), (14, None), (15, None), (2, 0), (3, 0), (3, 257), (5, 0), (6, 0.0), (7, 0), (13, 0)]
    for k, v in bad:
        a = list(args)
        a[k] = v
        assert L.asl_calibrate_lens_batch(*a) == -1, (k, v)
        assert L.asl_calibrate_lens_frames_device(*a, None) == -1, (k, v)
    assert (res == 0xAB).all() and (poses == 0xAB).all()
    assert L.asl_calibrate_lens_batch(*args) == 0                                      # and the call they were made from is fine
    assert res.view(CALIB_RESULT_DTYPE)[0]["status"] == 0
    brown5 = list(args)
    brown5[10], brown5[11], brown5[12] = 0, 5, 4                                       # what the fisheye refuses, the Brown lens takes
    assert L.asl_calibrate_lens_batch(*brown5) == 0
    with pytest.raises(ValueError):
        gpu_detector.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, n_dist=5, model="fisheye")
    with pytest.raises(_lib.AslError):
        gpu_detector.calibrate(obs, rec, LC.TAG_INNER, FC.W, FC.H, n_dist=4, flags=FR.ZERO_TANGENT_DIST, model="fisheye")


@pytest.fixture(scope="module")
def end_to_end():
    """the ray-traced fisheye frames through TagDetector.calibrate(lens_model="fisheye")"""
    from aprilslam_amd.tag_detector import TagDetector
    td = TagDetector({"camera_matrix": np.eye(3), "dist_coeffs": np.zeros(4)}, tag_size=LC.TAG_INNER, id_limit=0)
    frames = FC.e2e_frames()
    cr = td.calibrate(frames, FC.e2e_map(), n_dist=4, lens_model="fisheye")
    return td, frames, cr


def test_end_to_end_matches_the_statement_and_the_true_lens(end_to_end):
    from aprilslam_amd.dist import pack_observations
    td, frames, cr = end_to_end
    assert isinstance(cr, CalibrationResult) and cr.ok and cr.lens_model == "fisheye" and cr.n_frames_used == len(frames)
    # the same packed observations through the statement
    dets, npf = td.detector._det.detect_host(np.ascontiguousarray(frames))
    npf = np.asarray(npf, dtype=np.int64)
    obs = pack_observations(dets, np.zeros(len(dets), dtype=_lib.POSE_DTYPE), npf, int(npf.max()))
    want = FR.calibrate(obs, FC.e2e_map().as_records(), LC.TAG_INNER, FC.W, FC.H, n_dist=4)
    assert_same((cr.record, cr.poses), want, 1e-7)
    f, c, fld = FC.lens_errors(cr.record)
    print("e2e", f, c, fld, cr.rms_px)
    rec = FC.recorded()
    assert f <= rec["e2e_f_rel"][1] and c <= rec["e2e_c_px"][1] and fld <= rec["e2e_field_px"][1]


def test_round_trip_calibrate_views_detector(end_to_end):
    from aprilslam_amd.tag_detector import TagDetector
    td, frames, cr = end_to_end
    vs = cr.view_set(3, 90, (640, 480))
    views = vs.rectify(td.detector._det, np.ascontiguousarray(frames[2]))
    assert views.shape == (3, 480, 640) and views.dtype == np.uint8 and views.std() > 0
    td2 = TagDetector(cr.camera_params, tag_size=LC.TAG_INNER, id_limit=0, lens_model=cr.camera_params["lens_model"], rectify=True,
                      rectified_K=vs.views[1][0])
    ids = [d["id"] for d in td2.detect(np.ascontiguousarray(frames[2]))]
    assert len(ids) >= 2 and set(ids) <= set(range(12)), ids
