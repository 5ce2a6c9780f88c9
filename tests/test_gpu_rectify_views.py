"""Rectification into rotated pinhole views on the device (k_rectify_views, asl_rectify_views_device /
asl_rectify_views_u8) against the NumPy statement tests/rectify_views_ref.py, byte for byte, and a fisheye camera end to end
through rectify.ViewSet and the rig solver.

The harness is that of test_gpu_rectify.py: padded rows and frames, guard bytes behind rows, frames and views, the source
unchanged afterwards, random bytes as the image, and the smallest shapes at which the kernel can go wrong.  The bounds of
the end-to-end tests are the ones tests/rectify_views_cases.py records, measured on the CPU with the oracle and the
statements."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import rectify_views_cases as VC
import rectify_views_ref as VR
from aprilslam_amd import _lib
from aprilslam_amd.rectify import ViewSet
from aprilslam_amd.tag_detector import TagDetector
from test_gpu_rectify import DIST as BROWN, GUARD, SRC_GUARD, camera, random_frames, run_device

pytestmark = pytest.mark.gpu

FISH4 = np.array([-0.03, 0.006, -0.001, 0.0001])
# (model, dist): the two fisheye forms and the Brown lens with every coefficient
LENSES = {"fisheye0": (VR.LENS_FISHEYE, None), "fisheye4": (VR.LENS_FISHEYE, FISH4), "brown5": (VR.LENS_BROWN, BROWN[5])}


def rodrigues(axis, deg):
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def fisheye_camera(w, h):
    """0.35 w pixels per radian: the frame's width is 164 degrees of the lens"""
    return np.array([[0.35 * w, 0.0, 0.5 * w + 0.3], [0.0, 0.37 * w, 0.5 * h - 0.4], [0.0, 0.0, 1.0]])


def views_for(lens, n_views, w_out, h_out):
    """n_views pinholes of about 80 degrees turned about a general axis: no entry of R is 0 or 1; under the Brown lens the
    turns are small enough for most of every view to stay in front of the source camera"""
    f = 0.6 * w_out
    Kn = np.array([[f, 0.0, 0.5 * w_out - 0.7], [0.0, 1.05 * f, 0.5 * h_out + 0.2], [0.0, 0.0, 1.0]])
    turns = {1: [35.0], 3: [-55.0, 7.0, 60.0]}[n_views]
    scale = 0.3 if lens == "brown5" else 1.0
    return [(Kn, rodrigues([0.15, 1.0, -0.1], scale * t)) for t in turns]


def run_views_device(det, frames, K, dist, model, views, w_out, h_out, fill=0, theta_max=None, row_pad=5, out_pad=3, frame_pad=11):
    """frames (n, h, w[, 3]) through asl_rectify_views_device with padded rows and frames -> (n_views, n, h_out, w_out), read
    from where the layout says view v of frame i lies; every byte of the destination outside the output pixels must keep
    its guard value, and the source its bytes"""
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
    nv = len(views)
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.full((nv * n * pitch_out,), GUARD, dtype=torch.uint8, device="cuda:0")
    det.rectify_views_device(d_src.data_ptr(), n, ch, w, h, d_dst.data_ptr(), K, dist, views, model=model, width_out=w_out, height_out=h_out,
                             theta_max=theta_max, fill=fill, stride=stride, frame_pitch=pitch, stride_out=stride_out, frame_pitch_out=pitch_out,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy(), src), "the source was written to"
    out = np.empty((nv, n, h_out, w_out), dtype=np.uint8)
    for v in range(nv):
        for f in range(n):
            at = (v * n + f) * pitch_out
            rows = got[at:at + stride_out * h_out].reshape(h_out, stride_out)
            out[v, f] = rows[:, :w_out]
            assert (rows[:, w_out:] == GUARD).all(), "bytes after a row were written (view %d, frame %d)" % (v, f)
            assert (got[at + stride_out * h_out:at + pitch_out] == GUARD).all(), "bytes after view %d, frame %d were written" % (v, f)
    return out


def assert_same(got, frames, K, dist, model, views, w_out, h_out, fill=0, theta_max=None):
    for f in range(len(frames)):
        want = VR.rectify_views(frames[f], K, dist, model, views, w_out, h_out, fill=fill, theta_max=theta_max)
        bad = np.argwhere(got[:, f] != want)
        assert len(bad) == 0, "frame %d: %d pixels differ, first (view, y, x) = %s: got %d, want %d" % (
            f, len(bad), bad[0], got[:, f][tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("out", [(33, 21), (130, 8)])
@pytest.mark.parametrize("src", [(37, 19), (131, 9)])
def test_edge_shapes(gpu_detector, src, out, ch, n_views, lens):
    """3 frames, stride = row + 5, stride_out = w_out + 3, both pitches 11 bytes more than a frame; the view-major layout
    is what run_views_device reads by"""
    (w, h), (w_out, h_out) = src, out
    frames = random_frames(3, w, h, ch, seed=w + ch)
    model, dist = LENSES[lens]
    K = camera(w, h) if model == VR.LENS_BROWN else fisheye_camera(w, h)
    views = views_for(lens, n_views, w_out, h_out)
    got = run_views_device(gpu_detector, frames, K, dist, model, views, w_out, h_out)
    assert_same(got, frames, K, dist, model, views, w_out, h_out)
    assert len(np.unique(got)) > 50  # images, not a constant
    if n_views == 3:
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("ch", [1, 3])
def test_aligned_rows_take_the_dword_stores(gpu_detector, ch):
    """no padding anywhere and widths of whole dwords: every store is a dword; 132 x 40 is five column tiles by two rows of blocks"""
    frames = random_frames(2, 136, 44, ch, seed=9)
    K = fisheye_camera(136, 44)
    views = views_for("fisheye4", 3, 132, 40)
    got = run_views_device(gpu_detector, frames, K, FISH4, VR.LENS_FISHEYE, views, 132, 40, row_pad=0, out_pad=0, frame_pad=0)
    assert_same(got, frames, K, FISH4, VR.LENS_FISHEYE, views, 132, 40)


@pytest.mark.parametrize("ch", [1, 3])
def test_beyond_90_degrees(gpu_detector, ch):
    """a 200 degree lens (18 px/rad on 64 x 48) and a view turned 120 degrees: part of the output has Z < 0.  The fisheye
    samples there, the Brown model gives fill, and theta_max cuts a ring to fill exactly where the statement does"""
    w, h, w_out, h_out = 64, 48, 34, 26
    frames = random_frames(2, w, h, ch, seed=11)
    frames[frames == 9] = 10                    # 9 is the fill: a pixel that holds it was not sampled
    K = np.array([[18.0, 0.0, 32.2], [0.0, 18.0, 23.7], [0.0, 0.0, 1.0]])
    Kn = np.array([[17.0, 0.0, 17.3], [0.0, 17.0, 12.8], [0.0, 0.0, 1.0]])
    R = rodrigues([0.0, 1.0, 0.0], 120.0)
    xs, ys = np.meshgrid(np.arange(w_out) + 0.5, np.arange(h_out) + 0.5)
    Z = R[2, 0] * ((xs - Kn[0, 2]) / Kn[0, 0]) + R[2, 1] * ((ys - Kn[1, 2]) / Kn[1, 1]) + R[2, 2]
    assert (Z < 0).sum() > 100 and (Z > 0).sum() > 100
    fish = run_views_device(gpu_detector, frames, K, FISH4, VR.LENS_FISHEYE, [(Kn, R)], w_out, h_out, fill=9)
    assert_same(fish, frames, K, FISH4, VR.LENS_FISHEYE, [(Kn, R)], w_out, h_out, fill=9)
    assert (fish[0, 0][Z < 0] != 9).sum() > 50, "rays behind the camera plane are sampled under the fisheye model"
    brown = run_views_device(gpu_detector, frames, K, None, VR.LENS_BROWN, [(Kn, R)], w_out, h_out, fill=9)
    assert_same(brown, frames, K, None, VR.LENS_BROWN, [(Kn, R)], w_out, h_out, fill=9)
    assert (brown[0, :, Z <= 0] == 9).all()
    for deg in (100.0, 95.0, 82.0):
        cut = run_views_device(gpu_detector, frames, K, FISH4, VR.LENS_FISHEYE, [(Kn, R)], w_out, h_out, fill=9, theta_max=np.radians(deg))
        assert_same(cut, frames, K, FISH4, VR.LENS_FISHEYE, [(Kn, R)], w_out, h_out, fill=9, theta_max=np.radians(deg))
        assert ((cut == 9) & (fish != 9)).any() and (cut != 9).any(), deg
    # theta_max = pi and 0 both mean no cut
    for tm in (np.pi, 0.0):
        assert np.array_equal(run_views_device(gpu_detector, frames, K, FISH4, VR.LENS_FISHEYE, [(Kn, R)], w_out, h_out, fill=9, theta_max=tm), fish)


@pytest.mark.parametrize("n_dist", [0, 4])
def test_the_axis(gpu_detector, n_dist):
    """cx' = x + 0.5 and cy' = y + 0.5 of an interior pixel with R = I: r == 0 there, and the sample is at (cx, cy)"""
    frames = random_frames(2, 64, 48, 1, seed=5)
    K = np.array([[40.0, 0.0, 30.0], [0.0, 40.0, 20.0], [0.0, 0.0, 1.0]])   # (cx, cy): the corner shared by four pixels
    Kn = np.array([[30.0, 0.0, 37.5], [0.0, 30.0, 13.5], [0.0, 0.0, 1.0]])
    dist = FISH4 if n_dist else None
    u, v = VR.source_coords(37.5, 13.5, K, dist, VR.LENS_FISHEYE, Kn, np.eye(3))
    assert (float(u), float(v)) == (30.0, 20.0)
    got = run_views_device(gpu_detector, frames, K, dist, VR.LENS_FISHEYE, [(Kn, np.eye(3))], 66, 30)
    assert_same(got, frames, K, dist, VR.LENS_FISHEYE, [(Kn, np.eye(3))], 66, 30)
    for f in range(2):
        assert got[0, f, 13, 37] == int(np.floor(frames[f, 19:21, 29:31].astype(np.float64).sum() / 4 + 0.5))


@pytest.mark.parametrize("n_dist", [0, 4, 5])
@pytest.mark.parametrize("ch", [1, 3])
def test_identity_view_under_brown_gives_the_bytes_of_rectify_frames_device(gpu_detector, ch, n_dist):
    w, h, w_out, h_out = 37, 19, 33, 21
    frames = random_frames(3, w, h, ch, seed=21)
    K = camera(w, h)
    Kn = np.array([[0.8 * K[0, 0] * w_out / w, 0.0, 0.5 * w_out - 0.7], [0.0, 0.8 * K[1, 1] * h_out / h, 0.5 * h_out + 0.2], [0.0, 0.0, 1.0]])
    want = run_device(gpu_detector, frames, K, BROWN[n_dist], Kn, w_out, h_out, fill=33)
    got = run_views_device(gpu_detector, frames, K, BROWN[n_dist], VR.LENS_BROWN, [(Kn, np.eye(3)), (Kn, None)], w_out, h_out, fill=33)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    assert (want == 33).any() and len(np.unique(want)) > 50


@pytest.mark.parametrize("ch", [1, 3])
def test_host_form_gives_the_same_bytes(gpu_detector, ch):
    frame = random_frames(1, 131, 9, ch, seed=3)[0]
    K = fisheye_camera(131, 9)
    views = views_for("fisheye4", 3, 130, 8)
    got = gpu_detector.rectify_views(frame, K, FISH4, views, model="fisheye", size=(130, 8), theta_max=1.5, fill=200)
    assert got.shape == (3, 8, 130)
    assert np.array_equal(got, run_views_device(gpu_detector, frame[None], K, FISH4, VR.LENS_FISHEYE, views, 130, 8, fill=200, theta_max=1.5)[:, 0])
    assert np.array_equal(got, VR.rectify_views(frame, K, FISH4, VR.LENS_FISHEYE, views, 130, 8, fill=200, theta_max=1.5))
    # padded host rows and views: the padding of the destination keeps its bytes
    src = np.full((9, 131 * ch + 5), SRC_GUARD, dtype=np.uint8)
    src[:, :131 * ch] = frame.reshape(9, -1)
    view_pitch = 8 * 133 + 7
    dst = np.full(3 * view_pitch, GUARD, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    Kc, dc, rec = np.ascontiguousarray(K), np.ascontiguousarray(FISH4), _lib.rectify_view_records(views)
    _lib.check(gpu_detector._L.asl_rectify_views_u8(gpu_detector._h, src.ctypes.data, ch, 131, 9, src.shape[1], dst.ctypes.data, 130, 8, 133, view_pitch,
                                                    Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 4, 1, rec.ctypes.data, 3, 1.5, 200))
    assert (src.reshape(9, -1)[:, 131 * ch:] == SRC_GUARD).all()
    for v in range(3):
        rows = dst[v * view_pitch:v * view_pitch + 8 * 133].reshape(8, 133)
        assert np.array_equal(rows[:, :130], got[v]) and (rows[:, 130:] == GUARD).all()
        assert (dst[v * view_pitch + 8 * 133:(v + 1) * view_pitch] == GUARD).all()


def _bad_calls():
    """(name, changes to the good call of test_argument_errors): what check_rectify_call refuses, then what the views add"""
    nan, inf = float("nan"), float("inf")
    bad = [("channels2", dict(channels=2)), ("channels0", dict(channels=0)), ("n_frames0", dict(n_frames=0)), ("w0", dict(w=0)), ("h_neg", dict(h=-1)),
           ("w_out0", dict(w_out=0)), ("h_out_neg", dict(h_out=-3)), ("stride", dict(stride=37 * 3 - 1)), ("stride_out", dict(stride_out=32)),
           ("frame_pitch", dict(frame_pitch=(37 * 3 + 5) * 19 - 1)), ("frame_pitch_out", dict(frame_pitch_out=36 * 21 - 1)),
           ("n_dist3", dict(n_dist=3)), ("n_dist6", dict(n_dist=6)), ("dist_null", dict(dist=None)), ("fill_neg", dict(fill=-1)), ("fill256", dict(fill=256)),
           ("K0_nan", dict(K_at=(0, nan))), ("K8_inf", dict(K_at=(8, inf))), ("dist_nan", dict(dist_at=(3, nan))), ("fx0", dict(K_at=(0, 0.0))),
           ("fy_neg", dict(K_at=(4, -1.0))),
           ("overlap_dst_in_src", dict(overlap=100)), ("overlap_src_in_dst", dict(overlap=-100)),
           # the source inside the LAST view's frames only: the destination range is that of all views
           ("overlap_last_view", dict(overlap=-(2 * 3 * (36 * 21 + 11) + 50))),
           ("lens_model2", dict(lens_model=2)), ("lens_model_neg", dict(lens_model=-1)), ("fisheye_n_dist5", dict(n_dist=5)),
           ("brown_n_dist3", dict(lens_model=0, n_dist=3)),
           ("n_views0", dict(n_views=0)), ("n_views17", dict(n_views=17)), ("n_views_neg", dict(n_views=-2)), ("views_null", dict(views=None)),
           ("theta_nan", dict(theta_max=nan)), ("theta_inf", dict(theta_max=inf)), ("theta_neg", dict(theta_max=-0.5)), ("theta_above_pi", dict(theta_max=3.2))]
    for k in (0, 2, 5):
        bad.append(("view_K%d_nan" % k, dict(view_K_at=(2, k, nan))))
    bad += [("view_K_inf", dict(view_K_at=(0, 8, inf))), ("view_fx0", dict(view_K_at=(1, 0, 0.0))), ("view_fy_neg", dict(view_K_at=(2, 4, -3.0))),
            ("view_R_nan", dict(view_R_at=(1, 4, nan))), ("view_R_inf", dict(view_R_at=(2, 0, inf))), ("view_R_scaled", dict(view_R_scale=(1, 1.00001))),
            ("view_R_sheared", dict(view_R_at=(2, 1, 0.3))), ("view_R_reflection", dict(view_R_flip=0)), ("view_R_zero", dict(view_R_scale=(2, 0.0)))]
    return bad


@pytest.mark.parametrize("name", [b[0] for b in _bad_calls()])
def test_argument_errors(gpu_detector, name):
    """every refused call returns ASL_EINVAL with a message and leaves the destination as it was, on both entry points"""
    import torch
    change = dict(_bad_calls())[name]
    dp = C.POINTER(C.c_double)
    a = dict(n_frames=3, channels=3, w=37, h=19, stride=37 * 3 + 5, frame_pitch=(37 * 3 + 5) * 19 + 11, w_out=33, h_out=21, stride_out=36,
             frame_pitch_out=36 * 21 + 11, n_dist=4, fill=0, lens_model=1, n_views=3, theta_max=1.7)
    K, dist = fisheye_camera(37, 19).ravel().copy(), FISH4.copy()
    rec = _lib.rectify_view_records(views_for("fisheye4", 3, 33, 21))
    if change.get("lens_model") == 0 or name == "n_dist6":
        dist = BROWN[5].copy()
    for key, arr in (("K_at", K), ("dist_at", dist)):
        if key in change:
            arr[change[key][0]] = change[key][1]
    if "view_K_at" in change:
        v, k, val = change["view_K_at"]
        rec["K"][v].reshape(-1)[k] = val
    if "view_R_at" in change:
        v, k, val = change["view_R_at"]
        rec["R"][v].reshape(-1)[k] = val
    if "view_R_scale" in change:
        rec["R"][change["view_R_scale"][0]] *= change["view_R_scale"][1]
    if "view_R_flip" in change:
        rec["R"][change["view_R_flip"]][:, 0] *= -1.0
    a.update({k: v for k, v in change.items() if k in a})
    room = 3 * 3 * max((37 * 3 + 5) * 19 + 11, 36 * 21 + 11)
    buf = torch.full((2 * room,), GUARD, dtype=torch.uint8, device="cuda:0")
    src_ptr, dst_ptr = buf.data_ptr(), buf.data_ptr() + room
    if "overlap" in change:  # the destination starts inside the source, or the source inside the destination
        src_ptr, dst_ptr = (buf.data_ptr(), buf.data_ptr() + change["overlap"]) if change["overlap"] > 0 else (buf.data_ptr() - change["overlap"], buf.data_ptr())
    dist_p = None if ("dist" in change and change["dist"] is None) else dist.ctypes.data_as(dp)
    views_p = None if ("views" in change and change["views"] is None) else rec.ctypes.data
    L, hdl = gpu_detector._L, gpu_detector._h
    rc = L.asl_rectify_views_device(hdl, C.c_void_p(src_ptr), a["n_frames"], a["channels"], a["w"], a["h"], a["stride"], a["frame_pitch"],
                                    C.c_void_p(dst_ptr), a["w_out"], a["h_out"], a["stride_out"], a["frame_pitch_out"], K.ctypes.data_as(dp), dist_p,
                                    a["n_dist"], a["lens_model"], views_p, a["n_views"], a["theta_max"], a["fill"], None)
    torch.cuda.synchronize()
    assert rc == -1 and len(L.asl_last_error()) > 0, (name, rc)
    assert (buf == GUARD).all().item(), "a refused call wrote to device memory"
    if name.startswith(("n_frames", "frame_pitch")) and name != "frame_pitch_out":
        return  # the host form takes one image and no source pitch
    host = np.full(2 * room, GUARD, dtype=np.uint8)
    hs, hd = host.ctypes.data, host.ctypes.data + room
    if "overlap" in change:
        over = change["overlap"] if name != "overlap_last_view" else -(2 * (36 * 21 + 11) + 50)  # one image: the last view is the third
        hs, hd = (host.ctypes.data, host.ctypes.data + over) if over > 0 else (host.ctypes.data - over, host.ctypes.data)
    rc = L.asl_rectify_views_u8(hdl, C.c_void_p(hs), a["channels"], a["w"], a["h"], a["stride"], C.c_void_p(hd), a["w_out"], a["h_out"], a["stride_out"],
                                a["frame_pitch_out"], K.ctypes.data_as(dp), dist_p, a["n_dist"], a["lens_model"], views_p, a["n_views"], a["theta_max"],
                                a["fill"])
    assert rc == -1 and len(L.asl_last_error()) > 0, (name, rc)
    assert (host == GUARD).all(), "a refused call wrote to host memory"


def test_the_good_call_of_the_argument_errors_is_accepted(gpu_detector):
    """the call test_argument_errors changes one thing of is itself legal, so every refusal there is the change's"""
    frames = random_frames(3, 37, 19, 3, seed=8)
    views = views_for("fisheye4", 3, 33, 21)
    got = run_views_device(gpu_detector, frames, fisheye_camera(37, 19), FISH4, VR.LENS_FISHEYE, views, 33, 21, theta_max=1.7)
    assert_same(got, frames, fisheye_camera(37, 19), FISH4, VR.LENS_FISHEYE, views, 33, 21, theta_max=1.7)


def test_legal_while_a_batch_is_pending(gpu_detector):
    import torch
    frames = random_frames(1, 64, 48, 3, seed=1)
    t = torch.from_numpy(frames).to("cuda:0")
    gpu_detector.submit_device(t.data_ptr(), 1, 3, 64, 48)
    try:
        K = fisheye_camera(37, 19)
        views = views_for("fisheye4", 3, 33, 21)
        src = random_frames(1, 37, 19, 1, seed=4)
        want = VR.rectify_views(src[0], K, FISH4, VR.LENS_FISHEYE, views, 33, 21)
        assert np.array_equal(gpu_detector.rectify_views(src[0], K, FISH4, views, size=(33, 21)), want)
        assert np.array_equal(run_views_device(gpu_detector, src, K, FISH4, VR.LENS_FISHEYE, views, 33, 21)[:, 0], want)
    finally:
        gpu_detector.collect()


# ---- end to end: the six-tag fisheye frame of rectify_views_cases.py, host-rendered and uploaded -------------------------
@pytest.fixture(scope="module")
def scene():
    """(detector, ViewSet, the frame on the device, obs (3, 1, MAX_TAGS) of ViewSet.observe_device)"""
    import torch
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    vs = VC.view_set()
    frame = torch.from_numpy(VC.fisheye_frame().copy()).to("cuda:0")
    obs = vs.observe_device(det, frame.data_ptr(), 1, 3, VC.W, VC.H, LC.TAG_INNER, VC.MAX_TAGS, stream=torch.cuda.current_stream().cuda_stream)
    yield det, vs, frame, obs
    det.close()


def slots(row):
    return [s for s in row if s["flags"] & 1]


def test_observe_device_finds_the_six_tags_and_their_poses(scene):
    det, vs, frame, obs = scene
    assert obs.shape == (3, 1, VC.MAX_TAGS) and obs.dtype == _lib.OBS_DTYPE
    assert [[int(s["id"]) for s in slots(obs[v, 0])] for v in range(3)] == [[0, 1], [2, 3], [4, 5]]
    # the views the detector ran on hold the statement's bytes
    want = VR.rectify_views(VC.fisheye_frame(), VC.K, VC.DIST, VR.LENS_FISHEYE, vs.views, *VC.SIZE)
    assert np.array_equal(vs._frames[:want.size].cpu().numpy().reshape(want.shape), want)
    rec, gt = VC.recorded(), VC.ground_truth()
    worst = dict(corner=0.0, trans=0.0, rot=0.0)
    for v, (Kn, R) in enumerate(vs.views):
        for s in slots(obs[v, 0]):
            assert s["flags"] & 2, "no pose for tag %d" % s["id"]
            ref = gt[int(s["id"])]
            T = np.vstack([s["T"].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
            worst["corner"] = max(worst["corner"], float(np.abs(s["corners"].reshape(4, 2) - VC.true_corners(Kn, R, ref)).max()))
            worst["trans"] = max(worst["trans"], VC.trans_err(VC.in_source(R, T), ref))
            worst["rot"] = max(worst["rot"], VC.rot_err(VC.in_source(R, T), ref))
    print("corners %.4f px (bound %.4f), per-tag pose %.5f / %.5f rad (bounds %.5f / %.5f)" % (
        worst["corner"], rec["corner_px"][1], worst["trans"], worst["rot"], rec["tag_trans_rel"][1], rec["tag_rot_rad"][1]))
    assert worst["corner"] <= rec["corner_px"][1]
    assert worst["trans"] <= rec["tag_trans_rel"][1]
    assert worst["rot"] <= rec["tag_rot_rad"][1]


def test_the_views_localise_as_a_rig(scene):
    """the six true poses as the map: the rig pose is the identity within the recorded bound, and no single view's own
    localisation is better than it by more than the recorded margin"""
    det, vs, _, obs = scene
    rec = VC.recorded()
    pose = vs.rig().localize(det, obs, VC.tag_map(), LC.TAG_INNER)[0]
    assert pose["status"] == 0 and pose["n_tags"] == 6
    et, er = VC.pose_errors(pose["T"])
    single = VC.single_view_errors(vs, obs, lambda v, o, Kn: det.localize(o, VC.tag_map(), Kn, None, LC.TAG_INNER))
    assert len(single) == 3
    print("rig pose %.5f units, %.6f rad (bounds %.5f, %.6f); single views %s" % (et, er, rec["rig_trans"][1], rec["rig_rot_rad"][1], single))
    assert et <= rec["rig_trans"][1] and er <= rec["rig_rot_rad"][1]
    assert et - min(e[0] for e in single) <= rec["margin_trans"][1]
    assert er - min(e[1] for e in single) <= rec["margin_rot_rad"][1]


def test_tag_detector_with_a_fisheye_is_the_view_set_with_that_one_view(scene):
    """TagDetector(lens_model="fisheye", rectify=True) with one 100 degree view, R = I, against ViewSet with that view"""
    import torch
    det, _, frame, _ = scene
    Kn = VC.one_view_K()
    td = TagDetector({"camera_matrix": VC.K, "dist_coeffs": VC.DIST}, tag_size=LC.TAG_INNER, id_limit=0, lens_model="fisheye", rectify=True,
                     rectified_K=Kn)
    dets, poses, npf = td.detect_batch_device(frame.data_ptr(), 1, 3, VC.W, VC.H)
    one = ViewSet(VC.K, VC.DIST, "fisheye", [(Kn, np.eye(3))], (VC.W, VC.H))
    obs = one.observe_device(det, frame.data_ptr(), 1, 3, VC.W, VC.H, LC.TAG_INNER, VC.MAX_TAGS, stream=torch.cuda.current_stream().cuda_stream)
    got = slots(obs[0, 0])
    assert list(npf) == [len(got)] and len(got) >= 2 and [int(d["id"]) for d in dets] == [int(s["id"]) for s in got]
    for d, p, s in zip(dets, poses, got):
        assert np.array_equal(d["corners"].astype(np.float32).ravel(), s["corners"])
        assert p["ok"] and np.array_equal(p["T"][:3].ravel(), s["T"])
    # the frame it detected on is the view's, and the host path gives the device path's detections
    want = VR.rectify_views(VC.fisheye_frame(), VC.K, VC.DIST, VR.LENS_FISHEYE, [(Kn, np.eye(3))], VC.W, VC.H)[0]
    assert np.array_equal(td._rect_buf[:VC.W * VC.H].cpu().numpy().reshape(VC.H, VC.W), want)
    assert np.array_equal(one.rectify(det, VC.fisheye_frame())[0], want)
    host = td.detect(VC.fisheye_frame())
    assert [h["id"] for h in host] == [int(d["id"]) for d in dets]
    for h, d in zip(host, dets):
        assert np.array_equal(h["lb-rb-rt-lt"], d["corners"])
