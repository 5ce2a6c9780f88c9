"""A detector of several families (asl_detector_create_families, k_decode_multi) against the statement multifam_ref.py on
the mixed sheets of multifam_cases; test_multifam_ref.py checks (without a GPU) that the statement finds exactly the
placed tags there and equals the merged single-family oracle runs.  Bars: test_gpu_families.same_as_oracle's -- ids,
hamming, order and n_per_frame exact, corners and centres within stage_check.CORNER_TOL, margins equal as float32."""
import ctypes as C

import numpy as np
import pytest

import family_cases as FC
import multifam_cases as MC
import multifam_ref
import oracle_lib as O
import stage_check
from aprilslam_amd import _lib, synth
from aprilslam_amd.apriltag import apriltag
from aprilslam_amd.tag_detector import TagDetector

pytestmark = pytest.mark.gpu

SET_IDS = list(MC.SETS)


def same_as_statement(dets, ref):
    assert [int(d["id"]) for d in dets] == [r["id"] for r in ref]
    for d, r in zip(dets, ref):
        assert int(d["hamming"]) == r["hamming"]
        assert np.abs(d["corners"] - r["corners"]).max() <= stage_check.CORNER_TOL
        assert np.abs(d["center"] - r["center"]).max() <= stage_check.CORNER_TOL
        assert np.float32(d["margin"]) == np.float32(r["margin"])


def detect(names, frames, decimate=1, maxhamming=1, id_base=None, **kw):
    det = _lib.Detector(list(MC.families(names)), decimate=decimate, maxhamming=maxhamming, id_base=id_base)
    try:
        return det.detect_host(frames, channels=1 if np.ndim(frames) == 3 else None, **kw)
    finally:
        det.close()


def check_frames(dets, npf, refs):
    assert list(npf) == [len(r) for r in refs]
    start = 0
    for r in refs:
        same_as_statement(dets[start:start + len(r)], r)
        start += len(r)


@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("key", SET_IDS)
def test_every_set_against_the_statement(key, decimate):
    names = MC.SETS[key]
    dets, npf = detect(names, MC.batch(names, decimate), decimate)
    check_frames(dets, npf, [MC.statement(names, decimate, f) for f in range(5)])
    assert len(dets) >= 5 * 6


@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("key", ["one_width", "two_widths", "four"])
def test_shaded_mixed_sheet_pins_the_shared_border_samples(key, decimate):
    names = MC.SETS[key]
    dets, npf = detect(names, MC.shaded(names, decimate)[None], decimate)
    ref = MC.statement(names, decimate, 0, shade=True)
    assert [r["id"] for r in ref] == MC.placed_ids(names, decimate)
    check_frames(dets, npf, [ref])


@pytest.mark.parametrize("name", FC.NAMES)
def test_one_family_through_the_new_entry_point(name):
    """id_base 0: the bytes of asl_detector_create_family's detector; id_base 1000: only the id column differs, by 1000"""
    fam, frames = FC.family(name), FC.batch(name, 1)
    one = _lib.Detector(fam, decimate=1)
    try:
        a, na = one.detect_host(frames, channels=1)
    finally:
        one.close()
    assert list(na) == [FC.n_tags(name, 1)] * 5
    b, nb = detect((name,), frames, id_base=[0])
    assert list(nb) == list(na) and b.tobytes() == a.tobytes()
    c, nc = detect((name,), frames, id_base=[1000])
    assert list(nc) == list(na) and np.array_equal(c["id"], a["id"] + 1000)
    c = c.copy()
    c["id"] -= 1000
    assert c.tobytes() == a.tobytes()


@pytest.mark.parametrize("key", ["one_width", "four"])
def test_order_of_the_table_does_not_matter(key):
    names, frames = MC.SETS[key], MC.batch(MC.SETS[key], 1)
    base = MC.id_bases(names)
    a, na = detect(names, frames, id_base=list(base))
    b, nb = detect(names[::-1], frames, id_base=list(base[::-1]))
    assert list(na) == list(nb) and len(a) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("decimate", [1, 2])
def test_alias_pair_keeps_both_detections_of_every_quad(decimate):
    names = MC.SETS["alias"]
    n = FC.n_tags("classic16", decimate)
    frames = MC.batch(names, decimate)[:4]
    dets, npf = detect(names, frames, decimate)
    assert list(npf) == [2 * n] * 4
    check_frames(dets, npf, [MC.statement(names, decimate, f) for f in range(4)])
    assert [int(i) for i in dets["id"][:2 * n]] == sorted(list(range(n)) + [24 + (k + 19) % 24 for k in range(n)])


def test_bgr_frames():
    """the CH = 3 instantiation of k_decode_multi"""
    names = MC.SETS["one_width"]
    frames = np.ascontiguousarray(np.repeat(MC.batch(names, 1)[:, :, :, None], 3, axis=3))
    dets, npf = detect(names, frames)
    fams, base = MC.families(names), MC.id_bases(names)
    check_frames(dets, npf, [multifam_ref.detect(O.bgr2gray(frames[f]), fams, base, 1) for f in range(5)])
    assert list(npf) == [len(MC.placed_ids(names, 1))] * 5


@pytest.mark.parametrize("maxhamming", [0, 2])
def test_damaged_sheet_at_other_maxhamming(maxhamming):
    names = MC.SETS["min_width"]
    ref = MC.statement(names, 1, MC.DAMAGED, maxhamming)
    assert len(ref) == (0 if maxhamming == 0 else len(MC.placed_ids(names, 1)))
    dets, npf = detect(names, MC.batch(names, 1)[MC.DAMAGED], maxhamming=maxhamming)
    check_frames(dets, npf, [ref])


def test_same_batch_twice_gives_the_same_bytes():
    names = MC.SETS["four"]
    det = _lib.Detector(list(MC.families(names)), decimate=2)
    try:
        a, na = det.detect_host(MC.batch(names, 2), channels=1)
        a, na = a.copy(), list(na)
        b, nb = det.detect_host(MC.batch(names, 2), channels=1)
    finally:
        det.close()
    assert na == list(nb) and len(a) and a.tobytes() == b.tobytes()


def test_fused_pose_and_packed_observations():
    """asl_detect_batch_pose_u8: a detection's pose is, byte for byte, the pose its family's own detector gives that tag;
    asl_pack_observations_device lays the frame's slots out in ascending global id."""
    names = MC.SETS["one_width"]
    fams, base = MC.families(names), MC.id_bases(names)
    frames = MC.batch(names, 1)
    K, dist, size = synth.camera_matrix(MC.WIDTH, MC.HEIGHT, 45.0), np.zeros(4), 0.05
    det = _lib.Detector(list(fams), decimate=1)
    try:
        dets, poses, npf = det.detect_host(frames, channels=1, K=K, dist=dist, tag_size=size)
        dets, poses = dets.copy(), poses.copy()
        want = {}
        for f, b in zip(fams, base):
            one = _lib.Detector(f, decimate=1)
            try:
                d1, p1, n1 = one.detect_host(frames, channels=1, K=K, dist=dist, tag_size=size)
            finally:
                one.close()
            for d, p in zip(d1, p1):
                want[(int(d["frame"]), int(d["id"]) + b)] = (d.copy(), p.tobytes())
        assert len(dets) == len(want) == 5 * len(MC.placed_ids(names, 1))
        for d, p in zip(dets, poses):
            d1, p1 = want[(int(d["frame"]), int(d["id"]))]
            assert p.tobytes() == p1
            assert d["corners"].tobytes() == d1["corners"].tobytes() and np.float32(d["margin"]) == np.float32(d1["margin"])
        # the packed records of the same batch, resident on the device
        import torch
        B, mt = len(frames), 32
        dev = torch.device("cuda", 0)
        d_frames = torch.from_numpy(np.array(frames)).to(dev)
        d_obs = torch.empty((B, mt, _lib.OBS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        det.submit_device(d_frames.data_ptr(), B, 1, MC.WIDTH, MC.HEIGHT, stream=st, K=K, dist=dist, tag_size=size)
        det.pack_observations_device(d_obs.data_ptr(), mt, stream=st)
        det.collect()
        obs = d_obs.cpu().numpy().view(_lib.OBS_DTYPE).reshape(B, mt)
        ids = MC.placed_ids(names, 1)
        for f in range(B):
            used = obs[f][obs[f]["flags"] != 0]
            assert [int(i) for i in used["id"]] == ids
    finally:
        det.close()


def test_family_of_and_the_id_limit():
    names = MC.SETS["four"]
    base = [1000, 0, 500, 65536 - 24]
    det = _lib.Detector(list(names), decimate=2, id_base=base)  # by registered name
    try:
        assert det.id_base == tuple(base) and [f.name for f in det.families] == list(names)
        dets, npf = det.detect_host(MC.batch(names, 2)[0])
        assert sorted(int(i) for i in dets["id"]) == MC.placed_ids(names, 2, base) and len(dets) >= 6
        placed = {base[f] + k: (f, k) for f, k in MC.placed(names, 2)}
        for i in dets["id"]:
            assert det.family_of(int(i)) == placed[int(i)]
        for bad in (24, 499, 1024, 65535 - 24, 65536, -1):
            with pytest.raises(_lib.AslError, match="in no family's range"):
                det.family_of(bad)
        L = _lib.load()
        for n in (0, 3, 24):
            assert L.asl_detector_set_id_limit(det._h, n) == -1 and b"4 families" in L.asl_last_error()
        again, _ = det.detect_host(MC.batch(names, 2)[0])
        assert again.tobytes() == dets.tobytes()  # the refusal changed nothing
    finally:
        det.close()
    one = _lib.Detector(FC.family("circle21"), decimate=2)
    try:
        assert one.family_of(7) == (0, 7)
        with pytest.raises(_lib.AslError, match="in no family's range"):
            one.family_of(24)
    finally:
        one.close()
    with pytest.raises(_lib.AslError, match="family 1: id_base range"):
        _lib.Detector(list(MC.families(MC.SETS["two_widths"])), id_base=[0, 10])
    h = C.c_void_p()
    assert _lib.load().asl_detector_create_families(None, None, 2, 1, 1, 2.0, 0.0, 1, 0, C.byref(h)) == -1 and not h


def test_python_entry_points_take_a_list_of_names():
    names = MC.SETS["two_widths"]
    MC.families(names)  # registered
    img = MC.batch(names, 2)[0]
    base = MC.id_bases(names)
    want = sorted((base[f] + k, names[f], k) for f, k in MC.placed(names, 2))
    found = apriltag(list(names)).detect(img)
    assert [(d["id"], d["family"], d["local_id"]) for d in found] == want
    assert set(found[0]) == {"hamming", "margin", "id", "center", "lb-rb-rt-lt", "family", "local_id"}
    assert set(apriltag(names[0]).detect(img)[0]) == {"hamming", "margin", "id", "center", "lb-rb-rt-lt"}  # one name: as before
    cam = {"camera_matrix": synth.camera_matrix(MC.WIDTH, MC.HEIGHT, 45.0), "dist_coeffs": np.zeros((4, 1))}
    td = TagDetector(cam, tag_type=list(names))
    found = td.detect(np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2)))
    assert [(d["id"], d["family"], d["local_id"]) for d in found] == want and all(td.get_pose(d)[0] for d in found)
    assert [(d["id"], d["family"]) for d in td.detect(img)] == [w[:2] for w in want]
