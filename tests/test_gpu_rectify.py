"""Lens rectification on the device (k_rectify, asl_rectify_frames_device / asl_rectify_u8) against the NumPy statement
tests/rectify_ref.py, byte for byte, and end to end through TagDetector(rectify=True) on streams rendered on the device.

Shapes are the smallest at which the kernel can go wrong: widths that end in a partial dword and a partial 32-column tile,
heights that end in a partial 8-row tile and need a second row of tiles, rows and frames at unaligned addresses (the byte
stores) and at aligned ones (the dword stores), random bytes as the image.  The bounds of the end-to-end tests are the ones
tests/rectify_cases.py records, measured on the CPU with the oracle and the statement."""
import ctypes as C

import numpy as np
import pytest

import calib_cases as CC
import localize_cases as LC
import rectify_cases as RC
import rectify_ref as RR
from aprilslam_amd import _lib, rectify, synth
from aprilslam_amd.tag_detector import TagDetector

pytestmark = pytest.mark.gpu

GUARD, SRC_GUARD = 0xA5, 0x5A
DIST = {0: None, 4: np.array([-0.2, 0.05, 0.01, -0.02]), 5: np.array([-0.2, 0.05, 0.01, -0.02, 0.03])}


def camera(w, h, f=0.9):
    return np.array([[f * w, 0.0, 0.5 * w + 0.3], [0.0, 1.1 * f * w, 0.5 * h - 0.4], [0.0, 0.0, 1.0]])


def random_frames(n, w, h, ch, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w) + ((3,) if ch == 3 else ()), dtype=np.uint8)


def run_device(det, frames, K, dist, K_new, w_out, h_out, fill=0, row_pad=5, out_pad=3, frame_pad=11):
    """frames (n, h, w[, 3]) through asl_rectify_frames_device with padded rows and frames -> (n, h_out, w_out); every
    byte of the destination outside the output pixels must keep its guard value"""
    import torch
    n, h, w = frames.shape[:3]
    ch = 1 if frames.ndim == 3 else 3
    stride = w * ch + row_pad
    pitch = stride * h + frame_pad
    src = np.full(n * pitch, SRC_GUARD, dtype=np.uint8)
    for f in range(n):
        src[f * pitch:f * pitch + stride * h].reshape(h, stride)[:, :w * ch] = frames[f].reshape(h, w * ch)
    stride_out = w_out + out_pad
    pitch_out = stride_out * h_out + frame_pad
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.full((n * pitch_out,), GUARD, dtype=torch.uint8, device="cuda:0")
    det.rectify_frames_device(d_src.data_ptr(), n, ch, w, h, d_dst.data_ptr(), K, dist, K_new=K_new, width_out=w_out, height_out=h_out,
                              fill=fill, stride=stride, frame_pitch=pitch, stride_out=stride_out, frame_pitch_out=pitch_out,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src), "the source was written to"
    out = np.empty((n, h_out, w_out), dtype=np.uint8)
    for f in range(n):
        rows = got[f * pitch_out:f * pitch_out + stride_out * h_out].reshape(h_out, stride_out)
        out[f] = rows[:, :w_out]
        assert (rows[:, w_out:] == GUARD).all(), "bytes after a row were written (frame %d)" % f
        assert (got[f * pitch_out + stride_out * h_out:(f + 1) * pitch_out] == GUARD).all(), "bytes after frame %d were written" % f
    return out


def assert_same(got, frames, K, dist, K_new, w_out, h_out, fill=0):
    for f in range(len(frames)):
        want = RR.rectify(frames[f], K, dist, K_new, w_out, h_out, fill=fill)
        bad = np.argwhere(got[f] != want)
        assert len(bad) == 0, "frame %d: %d pixels differ, first (y, x) = %s: got %d, want %d" % (
            f, len(bad), bad[0], got[f][tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("n_dist", [0, 4, 5])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("out", [(33, 21), (130, 8)])
@pytest.mark.parametrize("src", [(37, 19), (131, 9)])
def test_edge_shapes(gpu_detector, src, out, ch, n_dist):
    """3 frames, stride = row + 5, stride_out = w_out + 3, both pitches 11 bytes more than a frame"""
    (w, h), (w_out, h_out) = src, out
    frames = random_frames(3, w, h, ch, seed=w + ch)
    K = camera(w, h)
    Kn = np.array([[0.8 * K[0, 0] * w_out / w, 0.0, 0.5 * w_out - 0.7], [0.0, 0.8 * K[1, 1] * h_out / h, 0.5 * h_out + 0.2], [0.0, 0.0, 1.0]])
    got = run_device(gpu_detector, frames, K, DIST[n_dist], Kn, w_out, h_out)
    assert_same(got, frames, K, DIST[n_dist], Kn, w_out, h_out)
    assert len(np.unique(got)) > 50  # an image, not a constant


@pytest.mark.parametrize("ch", [1, 3])
def test_aligned_rows_take_the_dword_stores(gpu_detector, ch):
    """no padding anywhere and widths of whole dwords: every store is a dword; 132 x 40 is five column tiles by two rows of blocks"""
    frames = random_frames(2, 136, 44, ch, seed=9)
    K = camera(136, 44)
    got = run_device(gpu_detector, frames, K, DIST[5], None, 132, 40, row_pad=0, out_pad=0, frame_pad=0)
    assert_same(got, frames, K, DIST[5], None, 132, 40)


@pytest.mark.parametrize("ch", [1, 3])
def test_gray_conversion_is_exact(gpu_detector, ch):
    """n_dist = 0, K_new = NULL, the same size: the source, or its gray conversion"""
    frames = random_frames(2, 37, 19, ch, seed=2)
    got = run_device(gpu_detector, frames, camera(37, 19), None, None, 37, 19)
    assert np.array_equal(got, frames if ch == 1 else RR.bgr_gray(frames))


@pytest.mark.parametrize("fill", [0, 200])
@pytest.mark.parametrize("ch", [1, 3])
def test_borders(gpu_detector, ch, fill):
    w, h = 37, 19
    frames = random_frames(2, w, h, ch, seed=7)
    K = camera(w, h)
    # a third of the output looks past the left edge of the source
    Kn = K.copy()
    Kn[0, 2] += w / 3.0
    got = run_device(gpu_detector, frames, K, DIST[4], Kn, w, h, fill=fill)
    assert_same(got, frames, K, DIST[4], Kn, w, h, fill=fill)
    assert (got[:, :, :10] == fill).all()
    # k1 = +8 throws everything but the centre outside: a tile's outline says nothing about its middle
    # (a short focal length of K_new spreads the output pixels: the tile x 0..31, y 8..15 has its corners and edge midpoints
    # outside and the pixels around (16, 12) inside)
    lens = np.array([8.0, 0.0, 0.0, 0.0])
    Kn = np.array([[2.0, 0.0, 16.2], [0.0, 2.0, 12.3], [0.0, 0.0, 1.0]])
    got = run_device(gpu_detector, frames, K, lens, Kn, 130, 40, fill=fill)
    assert_same(got, frames, K, lens, Kn, 130, 40, fill=fill)
    uv = RR.distort_points(np.array([[x + 0.5, y + 0.5] for y in (8, 12, 15) for x in (0, 16, 31)]), K, lens, Kn)
    inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
    assert list(inside) == [False] * 4 + [True] + [False] * 4
    # samples exactly at u = 0 (inside) and u = w (outside), then just below 0 (outside) and just below w (inside)
    eps = 2.0 ** -40
    Kh = np.array([[4.0, 0.0, 0.5], [0.0, 4.0, 0.5], [0.0, 0.0, 1.0]])
    for c0, first, last in ((0.0, 0.0, float(w)), (-eps, -eps, w - eps)):
        Ke = np.array([[2.0, 0.0, c0], [0.0, 2.0, c0], [0.0, 0.0, 1.0]])
        ends = RR.distort_points(np.array([[0.5, 0.5], [2 * w + 0.5, 0.5]]), Ke, None, Kh)
        assert ends[0, 0] == first and ends[1, 0] == last
        got = run_device(gpu_detector, frames, Ke, None, Kh, 2 * w + 2, 2 * h + 2, fill=fill)
        assert_same(got, frames, Ke, None, Kh, 2 * w + 2, 2 * h + 2, fill=fill)


@pytest.mark.parametrize("ch", [1, 3])
def test_host_form_gives_the_same_bytes(gpu_detector, ch):
    frame = random_frames(1, 131, 9, ch, seed=3)[0]
    K = camera(131, 9)
    Kn = camera(130, 8, f=0.7)
    got = gpu_detector.rectify(frame, K, DIST[5], K_new=Kn, size=(130, 8), fill=200)
    assert np.array_equal(got, run_device(gpu_detector, frame[None], K, DIST[5], Kn, 130, 8, fill=200)[0])
    assert np.array_equal(got, RR.rectify(frame, K, DIST[5], Kn, 130, 8, fill=200))
    # padded host rows: the padding of the destination keeps its bytes
    src = np.full((9, 131 * ch + 5), SRC_GUARD, dtype=np.uint8)
    src[:, :131 * ch] = frame.reshape(9, -1)
    dst = np.full((8, 133), GUARD, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    Kc, Knc, dc = np.ascontiguousarray(K), np.ascontiguousarray(Kn), np.ascontiguousarray(DIST[5])
    _lib.check(gpu_detector._L.asl_rectify_u8(gpu_detector._h, src.ctypes.data, ch, 131, 9, src.shape[1], dst.ctypes.data, 130, 8, 133,
                                              Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, Knc.ctypes.data_as(dp), 200))
    assert np.array_equal(dst[:, :130], got) and (dst[:, 130:] == GUARD).all()


def _bad_calls():
    """(name, changes to the good call of test_argument_errors)"""
    nan, inf = float("nan"), float("inf")
    bad = [("channels2", dict(channels=2)), ("channels0", dict(channels=0)), ("channels4", dict(channels=4)),
           ("n_frames0", dict(n_frames=0)), ("w0", dict(w=0)), ("h_neg", dict(h=-1)), ("w_out0", dict(w_out=0)), ("h_out_neg", dict(h_out=-3)),
           ("stride", dict(stride=37 * 3 - 1)), ("stride_out", dict(stride_out=32)), ("frame_pitch", dict(frame_pitch=(37 * 3 + 5) * 19 - 1)),
           ("frame_pitch_out", dict(frame_pitch_out=36 * 21 - 1)),
           ("n_dist3", dict(n_dist=3)), ("n_dist6", dict(n_dist=6)), ("n_dist1", dict(n_dist=1)), ("dist_null", dict(dist=None)),
           ("fill_neg", dict(fill=-1)), ("fill256", dict(fill=256)), ("overlap_dst_in_src", dict(overlap=100)), ("overlap_src_in_dst", dict(overlap=-100))]
    for k in (0, 2, 4, 8):
        bad.append(("K%d_nan" % k, dict(K_at=(k, nan))))
        bad.append(("K_new%d_inf" % k, dict(K_new_at=(k, inf))))
    bad += [("dist_nan", dict(dist_at=(4, nan))), ("dist_inf", dict(dist_at=(0, -inf))),
            ("fx0", dict(K_at=(0, 0.0))), ("fy_neg", dict(K_at=(4, -1.0))), ("fx_new_neg", dict(K_new_at=(0, -2.0))), ("fy_new0", dict(K_new_at=(4, 0.0)))]
    return bad


@pytest.mark.parametrize("name", [b[0] for b in _bad_calls()])
def test_argument_errors(gpu_detector, name):
    """every refused call returns ASL_EINVAL with a message and leaves the destination as it was, on both entry points"""
    import torch
    change = dict(_bad_calls())[name]
    dp = C.POINTER(C.c_double)
    a = dict(n_frames=3, channels=3, w=37, h=19, stride=37 * 3 + 5, frame_pitch=(37 * 3 + 5) * 19 + 11, w_out=33, h_out=21, stride_out=36,
             frame_pitch_out=36 * 21 + 11, n_dist=5, fill=0)
    K, Kn, dist = camera(37, 19).ravel().copy(), camera(33, 21).ravel().copy(), DIST[5].copy()
    for key, arr in (("K_at", K), ("K_new_at", Kn), ("dist_at", dist)):
        if key in change:
            arr[change[key][0]] = change[key][1]
    a.update({k: v for k, v in change.items() if k in a})
    room = 3 * max((37 * 3 + 5) * 19 + 11, 36 * 21 + 11)
    buf = torch.full((2 * room,), GUARD, dtype=torch.uint8, device="cuda:0")
    src_ptr, dst_ptr = buf.data_ptr(), buf.data_ptr() + room
    if "overlap" in change:  # the destination starts inside the source, or the source inside the destination
        src_ptr, dst_ptr = (buf.data_ptr(), buf.data_ptr() + change["overlap"]) if change["overlap"] > 0 else (buf.data_ptr() - change["overlap"], buf.data_ptr())
    dist_p = None if ("dist" in change and change["dist"] is None) else dist.ctypes.data_as(dp)
    L, hdl = gpu_detector._L, gpu_detector._h
    rc = L.asl_rectify_frames_device(hdl, C.c_void_p(src_ptr), a["n_frames"], a["channels"], a["w"], a["h"], a["stride"], a["frame_pitch"],
                                     C.c_void_p(dst_ptr), a["w_out"], a["h_out"], a["stride_out"], a["frame_pitch_out"], K.ctypes.data_as(dp), dist_p,
                                     a["n_dist"], Kn.ctypes.data_as(dp), a["fill"], None)
    torch.cuda.synchronize()
    assert rc == -1 and len(L.asl_last_error()) > 0, (name, rc)
    assert (buf == GUARD).all().item(), "a refused call wrote to device memory"
    if name.startswith(("n_frames", "frame_pitch")):
        return  # the host form takes one image and no pitches
    host = np.full(2 * room, GUARD, dtype=np.uint8)
    hs, hd = host.ctypes.data, host.ctypes.data + room
    if "overlap" in change:
        hs, hd = (host.ctypes.data, host.ctypes.data + change["overlap"]) if change["overlap"] > 0 else (host.ctypes.data - change["overlap"], host.ctypes.data)
    rc = L.asl_rectify_u8(hdl, C.c_void_p(hs), a["channels"], a["w"], a["h"], a["stride"], C.c_void_p(hd), a["w_out"], a["h_out"], a["stride_out"],
                          K.ctypes.data_as(dp), dist_p, a["n_dist"], Kn.ctypes.data_as(dp), a["fill"])
    assert rc == -1 and len(L.asl_last_error()) > 0, (name, rc)
    assert (host == GUARD).all(), "a refused call wrote to host memory"


def test_legal_while_a_batch_is_pending(gpu_detector):
    import torch
    frames = random_frames(1, 64, 48, 3, seed=1)
    t = torch.from_numpy(frames).to("cuda:0")
    gpu_detector.submit_device(t.data_ptr(), 1, 3, 64, 48)
    try:
        K = camera(37, 19)
        src = random_frames(1, 37, 19, 1, seed=4)
        assert np.array_equal(gpu_detector.rectify(src[0], K, DIST[4]), RR.rectify(src[0], K, DIST[4], None, 37, 19))
        assert_same(run_device(gpu_detector, src, K, DIST[4], None, 37, 19), src, K, DIST[4], None, 37, 19)
    finally:
        gpu_detector.collect()


# ---- end to end, the frames rendered on the device ------------------------------------------------------------------
def render_device(det, tags, cams, fov, dist):
    """(n, H, W, 3) BGR frames on the device, and the ground truth per frame"""
    import torch
    dev = torch.device("cuda:0")
    planes, gts = synth.render_planes(RC.W, RC.H, tags, LC.TAG_OUTER, cams, fov_y_deg=fov, dist=dist)
    tex = synth.gray_textures([int(t["id"]) for t in tags])
    d_tex = torch.from_numpy(tex).to(dev)
    d_planes = torch.from_numpy(planes.view(np.uint8).reshape(planes.shape + (-1,))).to(dev)
    frames = torch.empty((len(cams), RC.H, RC.W, 3), dtype=torch.uint8, device=dev)
    det.render_frames_device(frames.data_ptr(), len(cams), RC.W, RC.H, d_planes.data_ptr(), planes.shape[1], d_tex.data_ptr(), tex.shape[2],
                             tex.shape[1], 0.5 * LC.TAG_OUTER, K=synth.camera_matrix(RC.W, RC.H, fov) if dist is not None else None, dist=dist,
                             stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return frames, gts


def by_frame(dets, poses, npf):
    """[{id: (corners, T)}] per frame"""
    out, start = [], 0
    for n in npf:
        out.append({int(d["id"]): (np.array(d["corners"]), np.array(p["T"])) for d, p in zip(dets[start:start + n], poses[start:start + n]) if p["ok"]})
        assert len(out[-1]) == n
        start += n
    return out


@pytest.fixture(scope="module")
def mild():
    """the 8 frames of the mild-lens stream on the device, path A (the lens in the PnP) and path B (rectified first)"""
    K = synth.camera_matrix(RC.W, RC.H, CC.WEBCAM_FOV)
    params = {"camera_matrix": K, "dist_coeffs": CC.WEBCAM_DIST}
    A = TagDetector(params, tag_size=LC.TAG_INNER, id_limit=0)
    B = TagDetector(params, tag_size=LC.TAG_INNER, id_limit=0, rectify=True)
    tags, cams = RC.mild_stream()
    frames, gts = render_device(A.detector._det, tags, cams, CC.WEBCAM_FOV, CC.WEBCAM_DIST)
    ra = A.detect_batch_device(frames.data_ptr(), len(cams), 3, RC.W, RC.H)
    rb = B.detect_batch_device(frames.data_ptr(), len(cams), 3, RC.W, RC.H)
    return K, params, frames, gts, A, B, ra, rb


def test_mild_lens_rectified_path_agrees_with_the_lens_in_the_pnp(mild):
    """A is the yardstick.  Bounds: rectify_cases.recorded(), twice what the oracle and the statement give on this stream"""
    K, _, _, gts, _, _, ra, rb = mild
    rec = RC.recorded()
    fa, fb = by_frame(*ra), by_frame(*rb)
    worst = dict(corner=0.0, trans=0.0, rot=0.0)
    for f, (a, b) in enumerate(zip(fa, fb)):
        assert sorted(a) == sorted(b) and len(a) >= 1, (f, sorted(a), sorted(b))
        for i in a:
            back = rectify.distort_points(b[i][0], K, CC.WEBCAM_DIST)
            worst["corner"] = max(worst["corner"], float(np.abs(back - a[i][0]).max()))
        et, er = RC.pose_excess({i: a[i][1] for i in a}, {i: b[i][1] for i in b}, gts[f])
        worst["trans"], worst["rot"] = max(worst["trans"], et), max(worst["rot"], er)
    print("mild lens: corners %.4f px (bound %.4f), pose excess %.5f / %.5f rad (bounds %.5f / %.5f)" % (
        worst["corner"], rec["mild_corner_px"][1], worst["trans"], worst["rot"], rec["mild_trans_excess_rel"][1], rec["mild_rot_excess_rad"][1]))
    assert worst["corner"] <= rec["mild_corner_px"][1]
    assert worst["trans"] <= rec["mild_trans_excess_rel"][1]
    assert worst["rot"] <= rec["mild_rot_excess_rad"][1]


def test_rectified_frames_are_the_statements_and_the_host_path_agrees(mild):
    """the buffer TagDetector detects on holds the statement's bytes; detect() of the host frame gives the device path's result"""
    K, _, frames, _, _, B, _, rb = mild
    host = frames[0].cpu().numpy()
    want = RR.rectify(host, K, CC.WEBCAM_DIST, None, RC.W, RC.H)
    assert np.array_equal(B._rect_buf[:RC.W * RC.H].cpu().numpy().reshape(RC.H, RC.W), want)
    assert np.array_equal(B.detector._det.rectify(host, K, CC.WEBCAM_DIST), want)
    dets = B.detect(host)
    first = by_frame(*rb)[0]
    assert [d["id"] for d in dets] == sorted(first)
    for d in dets:
        assert np.array_equal(d["lb-rb-rt-lt"], first[d["id"]][0])
        ok, _, _, T = B.get_pose(d)
        assert ok and np.allclose(T, B.get_pose(dict(d, _pose=None))[3], rtol=0, atol=1e-9)  # the pose that rode along = a fresh PnP with rectified_K
    with pytest.raises(ValueError):
        B.calibrate(host[None], None)


def test_rectify_false_is_the_detector_without_the_keyword(mild):
    _, params, frames, _, A, _, ra, _ = mild
    off = TagDetector(params, tag_size=LC.TAG_INNER, id_limit=0, rectify=False)
    got = off.detect_batch_device(frames.data_ptr(), frames.shape[0], 3, RC.W, RC.H)
    for g, w in zip(got, ra):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
    host = frames[1].cpu().numpy()
    da, do = A.detect(host), off.detect(host)
    assert [d["id"] for d in da] == [d["id"] for d in do] and len(da) >= 1
    for x, y in zip(da, do):
        assert np.array_equal(x["lb-rb-rt-lt"], y["lb-rb-rt-lt"])
        assert all(np.array_equal(p, q) for p, q in zip(A.get_pose(x), off.get_pose(y)))
    assert all(np.array_equal(p, q) for p, q in zip(A.get_poses(da), off.get_poses(do)))


def test_wide_angle_lens():
    """the scene test_rectify_ref.py chose: the rectified path finds every tag and no other id, and every pose is within the
    recorded bound of the pose the same detector gives on the pinhole render of the scene"""
    _, fov, dist, fov_new, seed = RC.WIDE_SCENE
    K, Kn = RC.cameras(fov, fov_new)
    tags = RC.scene_tags(fov_new, seed)
    cams = [((0, 0, 0), (0, 0, 0))]
    P = TagDetector({"camera_matrix": Kn, "dist_coeffs": np.zeros(0)}, tag_size=LC.TAG_INNER, id_limit=0)
    B = TagDetector({"camera_matrix": K, "dist_coeffs": dist}, tag_size=LC.TAG_INNER, id_limit=0, rectify=True, rectified_K=Kn)
    pin, _ = render_device(P.detector._det, tags, cams, fov_new, None)
    raw, _ = render_device(P.detector._det, tags, cams, fov, dist)
    fp = by_frame(*P.detect_batch_device(pin.data_ptr(), 1, 3, RC.W, RC.H))[0]
    fb = by_frame(*B.detect_batch_device(raw.data_ptr(), 1, 3, RC.W, RC.H))[0]
    assert sorted(fb) == sorted(int(t["id"]) for t in tags) == sorted(fp)
    rec = RC.recorded()
    et = max(RC.trans_err(fb[i][1], fp[i][1]) for i in fb)
    er = max(RC.rot_err(fb[i][1], fp[i][1]) for i in fb)
    print("wide angle: translation %.5f (bound %.5f), rotation %.5f rad (bound %.5f)" % (et, rec["wide_trans_rel"][1], er, rec["wide_rot_rad"][1]))
    assert et <= rec["wide_trans_rel"][1] and er <= rec["wide_rot_rad"][1]
