"""Several sequences per call on the device (asl_smooth_sequences_device / _batch, k_smooth.inc): every sequence of a batch is,
byte for byte, what the single-sequence call with the covariance writes for its frames alone on the same build -- poses,
result record and covariance records.  The batches are those of tests/smooth_seq_cases.py; "alone" is det.smooth(...,
with_cov=True) of the sequence's frames."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as LC
import smooth_cases as SC
import smooth_seq_cases as SQ
import test_gpu_smooth as TG
from aprilslam_amd import _lib, synth
from aprilslam_amd._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE

pytestmark = pytest.mark.gpu


def together(det, b, with_cov=True, seed="given"):
    return det.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters,
                                seed=b.seed if seed == "given" else None, with_cov=with_cov)


def alone(det, b, k):
    a0, a1 = SQ.ranges(b)[k]
    return det.smooth(b.obs[a0:a1], b.rec, SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters, seed=b.seed[a0:a1], with_cov=True)


def assert_each_alone(det, b, got, which=None):
    """every sequence of the batched result against the call alone: bytes.  -> the results alone"""
    poses, results, cov = got
    assert poses.shape == (len(b.obs),) and results.shape == (len(b.seq_start) - 1,) and cov.shape == (len(b.obs),)
    singles = {}
    for k, (a0, a1) in enumerate(SQ.ranges(b)):
        if which is not None and k not in which:
            continue
        p1, r1, c1 = singles[k] = alone(det, b, k)
        assert poses[a0:a1].tobytes() == p1.tobytes(), ("poses", k, a0, a1)
        assert results[k].tobytes() == r1.tobytes(), ("result", k, results[k], r1)
        assert cov[a0:a1].tobytes() == c1.tobytes(), ("cov", k, a0, a1)
    return singles


@pytest.mark.parametrize("name", ["4", "1", "dist"])
def test_ragged_batch_against_the_calls_alone(gpu_detector, name):
    """lengths 1, 2, 3, 5, 64, 65, 130 at offsets that are no multiples of the kernels' 64-frame chunks; with one tag a frame
    the chain flips mirrored seeds inside the batch; the lens coefficients"""
    b = SQ.ragged_dist() if name == "dist" else SQ.ragged(int(name))
    got = together(gpu_detector, b)
    assert_each_alone(gpu_detector, b, got)
    for (a0, a1), case, res in zip(SQ.ranges(b), SQ.ragged_names(name), got[1]):
        TG.assert_same(case, got[0][a0:a1], res)
    if name == "1":
        assert got[1]["n_flipped"].sum() > 0
    assert (got[2]["status"] == 0).all()


def test_sequences_stop_apart(gpu_detector):
    b = SQ.stop_apart()
    got = together(gpu_detector, b)
    assert_each_alone(gpu_detector, b, got)
    trials = got[1]["iterations"].tolist()
    print("trials", trials)
    assert (got[1]["status"] == 0).all() and all(1 <= t < b.max_iters for t in trials)
    assert len(set(trials)) >= 2, trials


def test_failures_stay_local(gpu_detector):
    b = SQ.failures()
    poses, results, cov = got = together(gpu_detector, b)
    assert_each_alone(gpu_detector, b, got)
    assert results["status"].tolist() == SQ.FAILURES_STATUS
    r = SQ.ranges(b)
    assert poses["status"][r[0][0]:r[0][1]].tolist() == [6, 0, 0, 6, 0, 0, 6]
    assert (poses["status"][r[1][0]:r[1][1]] == 4).all() and (poses["status"][r[3][0]:r[3][1]] == 4).all()
    assert (poses["status"][r[2][0]:r[2][1]] == 1).all() and all(np.array_equal(T, np.eye(4)) for T in poses["T"][r[2][0]:r[2][1]])
    for (a0, a1), want in zip(r, SQ.FAILURES_COV_STATUS):
        assert (cov["status"][a0:a1] == want).all(), (a0, a1, want, cov["status"][a0:a1])
    assert poses[r[0][0]:r[0][1]].tobytes() == poses[r[4][0]:r[4][1]].tobytes()
    assert results[0].tobytes() == results[4].tobytes() and cov[r[0][0]:r[0][1]].tobytes() == cov[r[4][0]:r[4][1]].tobytes()


def test_many_short_sequences(gpu_detector):
    """390 sequences of one frame (more workgroups than CUs), and the same frames cut 1, 2, 3, 5, ..."""
    b = SQ.many_short()
    poses, results, cov = got = together(gpu_detector, b)
    assert_each_alone(gpu_detector, b, got, which=range(130))
    for rep in (1, 2):
        s = slice(130 * rep, 130 * (rep + 1))
        assert poses[s].tobytes() == poses[:130].tobytes() and results[s].tobytes() == results[:130].tobytes()
        assert cov[s].tobytes() == cov[:130].tobytes()
    p = SQ.short_pattern()
    assert_each_alone(gpu_detector, p, together(gpu_detector, p))


@pytest.mark.parametrize("n_seq", [SQ.SEQ_CHUNK, SQ.SEQ_CHUNK + 1, 910])
def test_more_sequences_than_one_launch_of_offsets_carries(gpu_detector, n_seq):
    """the offsets travel SEQ_CHUNK sequences a launch: one full launch, one sequence into the second, and 910"""
    b = SQ.past_one_chunk(n_seq)
    assert len(b.seq_start) == n_seq + 1
    poses, results, cov = got = together(gpu_detector, b)
    # the first 130 against the calls alone, and the last ones (across the edge of the first launch) too
    assert_each_alone(gpu_detector, b, got, which=list(range(130)) + list(range(n_seq - 20, n_seq)))
    for k in range(130, n_seq):     # every later sequence is one of the first 130 again
        assert poses[k].tobytes() == poses[k % 130].tobytes() and results[k].tobytes() == results[k % 130].tobytes(), k
        assert cov[k].tobytes() == cov[k % 130].tobytes(), k


class OnDevice:
    """a batch on device buffers, the output buffers in any number of copies"""

    def __init__(self, det, b, n_seq_max=None):
        import torch
        self.torch, self.det, self.b = torch, det, b
        self.dev = torch.device("cuda:0")
        self.n, self.mt = b.obs.shape
        self.d_obs = torch.from_numpy(np.ascontiguousarray(b.obs).view(np.uint8).reshape(-1)).to(self.dev)
        self.d_map = torch.from_numpy(b.rec.view(np.uint8)).to(self.dev)
        self.d_seed = torch.from_numpy(np.ascontiguousarray(b.seed).view(np.uint8).reshape(-1)).to(self.dev)
        self.n_seq_max = n_seq_max or len(b.seq_start) - 1
        self.stream = torch.cuda.Stream(self.dev)

    def outputs(self, fill=0):
        t = self.torch
        out = [t.full((size,), fill, dtype=t.uint8, device=self.dev)
               for size in (self.n * CAM_POSE_DTYPE.itemsize, self.n_seq_max * SMOOTH_RESULT_DTYPE.itemsize, self.n * POSE_COV_DTYPE.itemsize)]
        t.cuda.synchronize()    # filled on another stream than the calls'
        return out

    def enqueue(self, seq_start, out, with_cov=True):
        b = self.b
        self.det.smooth_sequences_device(self.d_obs.data_ptr(), self.n, self.mt, self.d_map.data_ptr(), len(b.rec), self.d_seed.data_ptr(),
                                         seq_start, out[0].data_ptr(), out[1].data_ptr(), SC.K, b.dist, SC.TAG, *b.sigmas,
                                         max_iters=b.max_iters, stream=self.stream.cuda_stream, cov_ptr=out[2].data_ptr() if with_cov else None)

    def single(self, out):
        """asl_smooth_cov_frames_device over all the frames as one sequence"""
        b = self.b
        self.det.smooth_device(self.d_obs.data_ptr(), self.n, self.mt, self.d_map.data_ptr(), len(b.rec), self.d_seed.data_ptr(),
                               out[0].data_ptr(), out[1].data_ptr(), SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters,
                               stream=self.stream.cuda_stream, cov_ptr=out[2].data_ptr())

    def fetch(self, out, n_seq):
        return (out[0].cpu().numpy().view(CAM_POSE_DTYPE), out[1].cpu().numpy().view(SMOOTH_RESULT_DTYPE)[:n_seq],
                out[2].cpu().numpy().view(POSE_COV_DTYPE))


def test_entry_points(gpu_detector):
    b = SQ.ragged_dist()
    dv = OnDevice(gpu_detector, b)
    n_seq = len(b.seq_start) - 1
    # one sequence through the new call is the single-sequence call
    o1, o2 = dv.outputs(), dv.outputs()
    dv.enqueue([0, dv.n], o1)
    dv.single(o2)
    dv.stream.synchronize()
    assert all(x.cpu().numpy()[:len(y)].tobytes() == y.cpu().numpy().tobytes() for x, y in zip(o1[:1] + o1[2:], o2[:1] + o2[2:]))
    assert o1[1].cpu().numpy()[:64].tobytes() == o2[1].cpu().numpy()[:64].tobytes()
    # without d_cov: the same poses and results
    full, plain = dv.outputs(), dv.outputs()
    dv.enqueue(b.seq_start, full)
    dv.enqueue(b.seq_start, plain, with_cov=False)
    dv.stream.synchronize()
    want = dv.fetch(full, n_seq)
    assert_each_alone(gpu_detector, b, want)
    assert plain[0].cpu().numpy().tobytes() == full[0].cpu().numpy().tobytes() and plain[1].cpu().numpy().tobytes() == full[1].cpu().numpy().tobytes()
    assert not plain[2].cpu().numpy().any()
    # the same call twice: the same bytes
    again = dv.outputs()
    dv.enqueue(b.seq_start, again)
    dv.stream.synchronize()
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(again, full))
    # the host form given the seeds, and seeding itself (seed == NULL) on the seeds of its own localisation
    host = together(gpu_detector, b)
    assert all(h.tobytes() == w.tobytes() for h, w in zip(host, want))
    own = gpu_detector.localize(b.obs, b.rec, SC.K, b.dist, SC.TAG)
    import torch
    dv.d_seed.copy_(torch.from_numpy(own.view(np.uint8).reshape(-1)))
    seeded = dv.outputs()
    dv.enqueue(b.seq_start, seeded)
    dv.stream.synchronize()
    host = together(gpu_detector, b, seed=None)
    assert all(h.tobytes() == w.tobytes() for h, w in zip(host, dv.fetch(seeded, n_seq)))
    assert not gpu_detector.smooth_sequences(b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, *b.sigmas, max_iters=b.max_iters)[1]["status"].any()


def test_permuting_the_sequences_permutes_the_outputs(gpu_detector):
    b = SQ.failures()
    base = together(gpu_detector, b)
    order = [3, 0, 4, 2, 1]
    r = SQ.ranges(b)
    p = SQ.join([(b.obs[r[k][0]:r[k][1]], b.seed[r[k][0]:r[k][1]]) for k in order], b.rec, b.dist, b.sigmas, b.max_iters)
    got = together(gpu_detector, p)
    for new, k in enumerate(order):
        (a0, a1), (c0, c1) = SQ.ranges(p)[new], r[k]
        assert got[0][a0:a1].tobytes() == base[0][c0:c1].tobytes() and got[2][a0:a1].tobytes() == base[2][c0:c1].tobytes()
        assert got[1][new].tobytes() == base[1][k].tobytes()


def test_back_to_back_calls_see_their_own_offsets(gpu_detector):
    """two calls on one stream, no wait between them, the offsets array overwritten in between"""
    b = SQ.ragged(4)
    other = SQ.join([(b.obs[a0:a1], b.seed[a0:a1]) for a0, a1 in ((0, 100), (100, 101), (101, 270))], b.rec, b.dist, b.sigmas, b.max_iters)
    dv = OnDevice(gpu_detector, b)
    o1, o2 = dv.outputs(0xAB), dv.outputs(0xAB)
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    Kc = np.ascontiguousarray(SC.K)
    start = np.zeros(len(b.seq_start), dtype=np.int32)

    def call(out, n_seq):
        return L.asl_smooth_sequences_device(gpu_detector._h, dv.d_obs.data_ptr(), dv.n, dv.mt, dv.d_map.data_ptr(), len(b.rec),
                                             Kc.ctypes.data_as(dp), None, 0, SC.TAG, dv.d_seed.data_ptr(),
                                             start.ctypes.data_as(C.POINTER(C.c_int32)), n_seq, *b.sigmas, b.max_iters, out[0].data_ptr(),
                                             out[1].data_ptr(), out[2].data_ptr(), dv.stream.cuda_stream)
    start[:] = b.seq_start
    assert call(o1, len(b.seq_start) - 1) == 0
    start[:len(other.seq_start)] = other.seq_start     # the caller's array is its own again
    assert call(o2, len(other.seq_start) - 1) == 0
    start[:] = -1
    dv.stream.synchronize()
    assert_each_alone(gpu_detector, b, dv.fetch(o1, len(b.seq_start) - 1))
    assert_each_alone(gpu_detector, other, dv.fetch(o2, len(other.seq_start) - 1))


def test_refusals_write_nothing(gpu_detector):
    import torch
    b = SQ.ragged_dist()
    dv = OnDevice(gpu_detector, b)
    out = dv.outputs(0xAB)
    n, mt, n_seq = dv.n, dv.mt, len(b.seq_start) - 1
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Kc, dc = np.ascontiguousarray(SC.K), np.ascontiguousarray(b.dist)
    Knan = Kc.copy()
    Knan[0, 0] = np.nan
    nan, inf = float("nan"), float("inf")
    keep = []

    def offsets(*v):
        keep.append(np.array(v, dtype=np.int32))
        return keep[-1].ctypes.data_as(ip)
    sig = b.sigmas
    #      0               1                     2  3   4                     5           6                      7
    ok = [gpu_detector._h, dv.d_obs.data_ptr(), n, mt, dv.d_map.data_ptr(), len(b.rec), Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp),
          # 8 9      10                    11              12     13      14      15      16 17                  18                  19
          5, SC.TAG, dv.d_seed.data_ptr(), offsets(0, 5, n), n_seq, sig[0], sig[1], sig[2], 5, out[0].data_ptr(), out[1].data_ptr(),
          out[2].data_ptr(), None]
    long = np.arange(0, 65536 * 2, 2, dtype=np.int32)    # 65536 sequences' offsets
    keep.append(long)
    # 1048577 frames in 17 sequences of at most 65535 frames each: only the bound on the frames of a call refuses it
    big = np.concatenate([np.arange(17, dtype=np.int64) * 65535, [1048577]]).astype(np.int32)
    assert np.diff(big).max() <= 65535 and np.diff(big).min() >= 1 and big[-1] == 1048577
    keep.append(big)
    too_many = (1048577, big.ctypes.data_as(ip), 17)
    single = [(1, None), (4, None), (6, None), (10, None), (17, None), (18, None), (3, 0), (3, 257), (8, 3), (7, None),
              (6, Knan.ctypes.data_as(dp)), (9, nan), (9, inf), (13, 0.0), (13, nan), (14, -1.0), (14, inf), (15, 0.0), (15, nan), (16, 0), (16, 101),
              (17, dv.d_seed.data_ptr()), (17, dv.d_seed.data_ptr() + 160 * (n - 1)), (19, out[0].data_ptr()), (19, dv.d_seed.data_ptr())]
    seqs = [(11, None), (12, 0), (12, -1), (12, 65536), (11, offsets(1, 5, n)), (11, offsets(0, 5, n - 1)), (11, offsets(0, 5, n + 1)),
            (11, offsets(0, 0, n)), (11, offsets(0, n, n)), (11, offsets(0, n + 1, n)), (11, offsets(0, -1, n)), (2, 0), (2, -1)]
    seed_before = dv.d_seed.cpu().numpy().tobytes()
    torch.cuda.synchronize()
    for k, v in single + seqs:
        a = list(ok)
        a[k] = v
        assert L.asl_smooth_sequences_device(*a) == -1, (k, v)
    # more frames in all than a call takes; one sequence longer than 65535 frames; more sequences than a call takes.  Refused
    # before a pointer is followed: the buffers here are far smaller
    for nf, st, ns in (too_many, (65536, offsets(0, 65536), 1), (65537, offsets(0, 1, 65537), 2)):
        a = list(ok)
        a[2], a[11], a[12] = nf, st, ns
        assert L.asl_smooth_sequences_device(*a) == -1, (nf, ns)
    a = list(ok)
    a[2], a[11], a[12] = 65536 * 2, long.ctypes.data_as(ip), 65536
    assert L.asl_smooth_sequences_device(*a) == -1
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == 0xAB).all() for o in out) and dv.d_seed.cpu().numpy().tobytes() == seed_before
    # the host form refuses the same way
    h_out = np.full(n * CAM_POSE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    h_res = np.full(n_seq * 64, 0xAB, dtype=np.uint8)
    h_cov = np.full(n * POSE_COV_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    obs, seed = np.ascontiguousarray(b.obs), np.ascontiguousarray(b.seed)
    hk = [gpu_detector._h, obs.ctypes.data, n, mt, b.rec.ctypes.data, len(b.rec), Kc.ctypes.data_as(dp), dc.ctypes.data_as(dp), 5, SC.TAG,
          seed.ctypes.data, offsets(0, 5, n), n_seq, sig[0], sig[1], sig[2], 5, h_out.ctypes.data, h_res.ctypes.data, h_cov.ctypes.data]
    host_single = [(k, v) for k, v in single if k not in (10, 17, 19)] + [(17, None)]   # the seed may be NULL; host arrays may not overlap by contract
    for k, v in host_single + seqs:
        a = list(hk)
        a[k] = v
        assert L.asl_smooth_sequences_batch(*a) == -1, (k, v)
    for nf, st, ns in (too_many, (65536, offsets(0, 65536), 1), (65537, offsets(0, 1, 65537), 2)):
        a = list(hk)
        a[2], a[11], a[12] = nf, st, ns
        assert L.asl_smooth_sequences_batch(*a) == -1, (nf, ns)
    assert (h_out == 0xAB).all() and (h_res == 0xAB).all() and (h_cov == 0xAB).all()
    # and a good call writes
    assert L.asl_smooth_sequences_device(*ok) == 0
    torch.cuda.synchronize()
    assert not any((o.cpu().numpy() == 0xAB).all() for o in out)
    assert L.asl_smooth_sequences_batch(*hk) == 0
    assert h_out.tobytes() == out[0].cpu().numpy().tobytes() and h_res.tobytes() == out[1].cpu().numpy().tobytes()
    assert h_cov.tobytes() == out[2].cpu().numpy().tobytes()


def test_tag_detector_and_slam_surface():
    """TagDetector.localize_sequences on what detect_host returns: two rendered sequences of different length, one with a blank
    frame, against localize_sequence of each alone"""
    from aprilslam_amd.localize import TagMap
    from aprilslam_amd.slam import SLAM
    from aprilslam_amd.smooth import SmoothResult
    from aprilslam_amd.tag_detector import TagDetector
    tags = LC.bench_scene()
    tm = TagMap.from_scene(tags)
    td = TagDetector({"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, id_limit=0)
    cams = LC.trajectory(520)[:5]
    frames = [synth.render_frame(LC.W, LC.H, tags, LC.TAG_OUTER, cam_position=p, cam_rotation_deg=r)[0] for p, r in cams]
    first = [frames[0], frames[1], np.zeros_like(frames[0]), frames[2]]
    second = [frames[3], frames[4]]
    seqs = [td.detector._det.detect_host(np.stack(f), K=SC.K, dist=np.zeros(4), tag_size=SC.TAG) for f in (first, second)]
    kw = dict(sigma_px=0.5, sigma_rot=0.01, sigma_trans=0.2)
    mt = max(int(np.max(s[2])) for s in seqs)
    got = td.localize_sequences(seqs, tm, **kw)
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(r, SmoothResult) for r in got)
    assert [len(r.poses) for r in got] == [4, 2] and got[0].poses["status"].tolist() == [0, 0, 6, 0] and got[1].poses["status"].tolist() == [0, 0]
    for r, s in zip(got, seqs):
        one = td.localize_sequence(*s, tm, max_tags=mt, **kw)
        assert r.ok and r.poses.tobytes() == one.poses.tobytes() and r.result.tobytes() == one.result.tobytes()
        assert r.seed.tobytes() == one.seed.tobytes() and not r.flipped.any()
    with_cov = td.localize_sequences(seqs, tm, with_cov=True, **kw)
    assert [r.cov.shape for r in with_cov] == [(4, 6, 6), (2, 6, 6)] and all((r.cov_status == 0).all() for r in with_cov)
    assert all(a.poses.tobytes() == c.poses.tobytes() for a, c in zip(got, with_cov))

    class _Log:
        def info(self, m):
            pass
    slam = SLAM(_Log(), {"camera_matrix": SC.K, "dist_coeffs": np.zeros(4)}, tag_size=SC.TAG, detector=td)
    for det in slam.detect(frames[0]):
        slam.get_pose(det)
    before = slam.graph.estimated_pose.copy()
    rs = slam.localize_sequences(seqs, **kw)
    assert len(rs) == 2 and all(r.ok for r in rs) and [r.trajectory().shape for r in rs] == [(4, 4, 4), (2, 4, 4)]
    assert np.array_equal(slam.graph.estimated_pose, before)
