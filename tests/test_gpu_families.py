"""A detector for any tag family table (asl_detector_create_family), against the CPU oracle on the sheets of
family_cases: six layouts that between them take every path a family chooses in the quad fit, k_refine and k_decode --
both border polarities, 40 to 64 border samples, with and without a centre bit, with and without the code-book index,
payload inside and outside the border, 8 x 8 to 10 x 10 grids.  test_family_tables.py checks (without a GPU) that the
oracle finds exactly the tags placed on these sheets.  The flat sheets do not show which border samples the gray
models were fitted to; the shaded sheets do (family_cases.shaded), for the five families with more than 40."""
import ctypes as C
import logging

import numpy as np
import pytest

import family_cases as FC
import oracle_lib as O
import stage_check
import tag_sheet
from aprilslam_amd import _lib, synth
from aprilslam_amd.apriltag import apriltag
from aprilslam_amd.families import TagFamily, get_family
from aprilslam_amd.slam import SLAM
from aprilslam_amd.tag_detector import TagDetector

pytestmark = pytest.mark.gpu


def same_as_oracle(dets, ref):
    """stage_check's bars for the detections of one frame"""
    assert [int(d["id"]) for d in dets] == [r["id"] for r in ref]
    for d, r in zip(dets, ref):
        assert int(d["hamming"]) == r["hamming"]
        assert np.abs(d["corners"] - r["corners"]).max() <= stage_check.CORNER_TOL
        assert np.abs(d["center"] - r["center"]).max() <= stage_check.CORNER_TOL
        assert np.float32(d["margin"]) == np.float32(r["margin"])


@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("name", FC.NAMES)
def test_every_stage_matches_the_oracle(name, decimate):
    """check_stages' bars: ids, hamming and order exact, corners within 1e-9 px, margins equal as float32."""
    fam = FC.family(name)
    det = _lib.Detector(fam, decimate=decimate)
    try:
        dets, npf = stage_check.check_stages(det, FC.batch(name, decimate), fam, decimate)
    finally:
        det.close()
    n = FC.n_tags(name, decimate)
    assert list(npf) == [n] * 5
    assert [int(h) for h in dets["hamming"]] == [0] * (4 * n) + [1] * n


@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("name", FC.NAMES)
def test_shaded_sheet_pins_the_border_sample_set(name, decimate):
    """Flat sheets cannot tell which border samples were fitted (family_cases.shaded says why); this one can."""
    fam = FC.family(name)
    det = _lib.Detector(fam, decimate=decimate)
    try:
        dets, npf = stage_check.check_stages(det, FC.shaded(name, decimate)[None], fam, decimate)
    finally:
        det.close()
    assert list(npf) == [FC.n_tags(name, decimate)] and not dets["hamming"].any()


@pytest.mark.parametrize("name", ["classic36", "std52"])
def test_bgr_frames(name):
    """the CH = 3 instantiation of k_decode"""
    fam = FC.family(name)
    frames = np.ascontiguousarray(np.repeat(FC.batch(name, 1)[:, :, :, None], 3, axis=3))
    det = _lib.Detector(name, decimate=1)  # by its registered name
    try:
        dets, npf = stage_check.check_stages(det, frames, fam, 1)
    finally:
        det.close()
    assert list(npf) == [FC.n_tags(name, 1)] * 5


@pytest.mark.parametrize("maxhamming", [0, 2])
@pytest.mark.parametrize("name", ["classic36", "std52"])
def test_damaged_sheet_at_other_maxhamming(name, maxhamming):
    fam = FC.family(name)
    ref = FC.oracle_detections(name, 1, FC.DAMAGED, maxhamming)
    assert len(ref) == (0 if maxhamming == 0 else FC.n_tags(name, 1))
    det = _lib.Detector(fam, decimate=1, maxhamming=maxhamming)
    try:
        dets, _ = det.detect_host(FC.batch(name, 1)[FC.DAMAGED])
    finally:
        det.close()
    same_as_oracle(dets, ref)


@pytest.mark.parametrize("name", ["classic36", "classic16", "custom48"])
def test_index_and_whole_book_search_agree(name, monkeypatch):
    fam = FC.family(name)
    frames = FC.batch(name, 1)
    out = []
    for no_index in (False, True):
        if no_index:
            monkeypatch.setenv("ASL_NO_CODE_INDEX", "1")
        det = _lib.Detector(fam, decimate=1, maxhamming=2 if name == "classic36" else 1)
        try:
            dets, npf = det.detect_host(frames, channels=1)
        finally:
            det.close()
        out.append((dets.tobytes(), list(npf)))
    assert out[0][1] == [FC.n_tags(name, 1)] * 5
    assert out[0] == out[1]


def test_shipped_table_as_a_callers_family(gpu_detector):
    """tagStandard41h12 handed in as data decodes what the named detector with its id limit open decodes, byte for byte."""
    fam = get_family("tagStandard41h12")
    d = fam.to_dict()
    d["name"] = "shipped41h12_as_data"
    img = tag_sheet.tag_sheet(fam, 256, 192, 6, 16, ids=lambda k: 100 + 37 * k)
    mine = _lib.Detector(TagFamily.from_dict(d))
    try:
        a, na = mine.detect_host(img)
    finally:
        mine.close()
    b, nb = gpu_detector.detect_host(img)
    assert list(na) == list(nb) == [6] and [int(i) for i in a["id"]] == [100 + 37 * k for k in range(6)]
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("detector,sheet", [("classic36", "std52"), ("std52", "classic36")])
def test_another_familys_sheet_holds_nothing(detector, sheet):
    fam = FC.family(detector)
    frames = FC.batch(sheet, 1)
    for f in range(5):
        assert O.detect_gray(frames[f], fam, 1) == []
    det = _lib.Detector(fam, decimate=1)
    try:
        dets, npf = det.detect_host(frames, channels=1)
    finally:
        det.close()
    assert len(dets) == 0 and list(npf) == [0] * 5


def test_id_limit_is_bounded_by_the_callers_table():
    fam = FC.family("circle21")
    det = _lib.Detector(fam, decimate=2)
    try:
        L, img = _lib.load(), FC.batch("circle21", 2)[0]
        assert [int(i) for i in det.detect_host(img)[0]["id"]] == list(range(6))  # every id by default
        assert L.asl_detector_set_id_limit(det._h, fam.ncodes + 1) == -1
        assert b"holds 24 ids" in L.asl_last_error()
        assert [int(i) for i in det.detect_host(img)[0]["id"]] == list(range(6))  # the refusal changed nothing
        assert L.asl_detector_set_id_limit(det._h, 3) == 0
        short = fam.to_dict()
        short["codes"] = short["codes"][:3]
        same_as_oracle(det.detect_host(img)[0], O.detect_gray(img, TagFamily.from_dict(short), 2))
        assert L.asl_detector_set_id_limit(det._h, fam.ncodes) == 0 and L.asl_detector_set_id_limit(det._h, 0) == 0
        assert [int(i) for i in det.detect_host(img)[0]["id"]] == list(range(6))
    finally:
        det.close()


def test_create_family_refuses_what_the_check_refuses():
    d = FC.family("classic36").to_dict()
    d["width_at_border"] = 9
    with pytest.raises(_lib.AslError, match="width_at_border"):
        _lib.Detector(TagFamily.from_dict(d))
    with pytest.raises(_lib.AslError, match="unknown tag family 'no_such_family'"):
        _lib.Detector("no_such_family")
    h = C.c_void_p()
    assert _lib.load().asl_detector_create_family(None, 1, 1, 2.0, 0.0, 1, 0, C.byref(h)) == -1 and not h


@pytest.mark.parametrize("name", ["classic25", "custom48"])
def test_the_python_entry_points_take_a_registered_name(name):
    fam = FC.family(name)
    img = FC.batch(name, 2)[0]
    ids = list(range(FC.n_tags(name, 2)))
    assert [d["id"] for d in apriltag(name).detect(img)] == ids
    cam = {"camera_matrix": synth.camera_matrix(FC.WIDTH, FC.HEIGHT, 45.0), "dist_coeffs": np.zeros((4, 1))}
    td = TagDetector(cam, tag_type=name)
    found = td.detect(np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2)))
    assert [d["id"] for d in found] == ids and all(td.get_pose(d)[0] for d in found)
    # a rendered scene of the family (synth.render_frame(family=name)) through SLAM(tag_type=name)
    sc = synth.default_scene()
    W, H = 640, 480
    frame, _ = synth.render_frame(W, H, sc["tags"], sc["tag_size_outer"] * sc["size_scale"], cam_position=(1.3, -0.7, 2.1),
                                  cam_rotation_deg=(1.0, -2.0, 0.5), family=name)
    ref = O.detect_bgr(frame, fam)
    assert len(ref) >= 2
    slam = SLAM(logging.getLogger("test_gpu_families"), {"camera_matrix": synth.camera_matrix(W, H, sc["fov_y"]),
                                                         "dist_coeffs": np.zeros((4, 1))}, tag_type=name)
    assert [d["id"] for d in slam.detect(frame)] == [r["id"] for r in ref]
