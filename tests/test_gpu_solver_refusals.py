"""What the solver entry points say when they refuse (csrc/solve_host.inc): for every family -- calibration, mapping, sequence
smoothing (plain, covariance, sequences), per-tag covariance, one localisation and one rig entry -- the valid call returns 0,
every single-fault call returns -1 with the literal asl_last_error() text and writes nothing, two-fault calls give the
message of the check that comes first, and the host and device forms of a solver say the same for the same fault.  The
library is called through ctypes directly on the smallest block there is: 2 frames x 1 empty slot, n_ids 1; nothing is
launched but the valid calls."""
import ctypes as C

import numpy as np
import pytest

from aprilslam_amd import _lib
from aprilslam_amd._lib import CALIB_RESULT_DTYPE, CAM_POSE_DTYPE, MAP_TAG_DTYPE, OBS_DTYPE, RIG_CAMERA_DTYPE

pytestmark = pytest.mark.gpu

N, MT, NI = 2, 1, 1
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
K = np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 1]])
KNAN = K.copy()
KNAN[1, 1] = np.nan
DIST = np.zeros(5)
KEEP = []    # arrays behind the pointers handed to ctypes

NULL_D, NULL_ARG = "NULL detector", "NULL argument"
MAX_TAGS = "max_tags must be in [1, 256] (got %d)"
N_IDS = "n_ids must be >= 1 (got 0)"
N_DIST = "n_dist must be 0, 4 or 5"
NO_DIST = "dist is NULL with n_dist = 4"
TAG_SIZE = "tag_size must be positive (got 0)"
SIGMA_PX = "sigma_px must be >= 0 and finite (got -1)"
SIGMAS = "sigma_px, sigma_rot and sigma_trans must be positive and finite (got 0)"
SMOOTH_ITERS = "max_iters must be in [1, 100] (got %d)"


def dptr(a):
    KEEP.append(np.ascontiguousarray(a, dtype=np.float64))
    return KEEP[-1].ctypes.data_as(DP)


def offsets(*v):
    KEEP.append(np.array(v, dtype=np.int32))
    return KEEP[-1].ctypes.data_as(IP)


class Form:
    """one entry point, its arguments by name, and the buffers it may write (device tensors or host arrays of 0x55)"""

    def __init__(self, name, names, base, outputs):
        self.fn, self.name, self.names, self.base, self.outputs = getattr(_lib.load(), name), name, names.split(), base, outputs
        assert set(self.names) == set(base), (name, set(self.names) ^ set(base))

    def __call__(self, **changes):
        assert set(changes) <= set(self.names), (self.name, changes)
        return self.fn(*[changes.get(n, self.base[n]) for n in self.names])

    def refuses(self, message, **changes):
        rc = self(**changes)
        said = _lib.load().asl_last_error().decode()
        assert (rc, said) == (-1, message), (self.name, changes, rc, said)

    def fill(self):
        for o in self.outputs:
            o.fill(0x55) if isinstance(o, np.ndarray) else o.fill_(0x55)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(((o if isinstance(o, np.ndarray) else o.cpu().numpy()) == 0x55).all() for o in self.outputs)


def run(form, single, pairs):
    """the valid call, then every refusal on outputs of 0x55"""
    assert form() == 0, (form.name, _lib.load().asl_last_error())
    form.fill()
    for message, changes in single + pairs:
        form.refuses(message, **changes)
    assert form.untouched(), form.name


@pytest.fixture(scope="module")
def block(gpu_detector):
    """the block, the map, a seed and a camera table, on the host and on the device; out(n, device): an output of n bytes of 0x55 on either"""
    import torch
    obs = np.zeros((N, MT), dtype=OBS_DTYPE)
    obs["id"] = -1
    tmap = np.zeros(NI, dtype=MAP_TAG_DTYPE)
    seed = np.zeros(N, dtype=CAM_POSE_DTYPE)    # what localisation writes for a frame without tags
    seed["T"], seed["status"] = np.eye(4), 1
    rig = np.zeros(1, dtype=RIG_CAMERA_DTYPE)
    rig["K"], rig["E"] = K, np.eye(4)[:3]

    def to_device(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")

    class B:
        h = gpu_detector._h
        host = dict(obs=obs, map=tmap, seed=seed, rig=rig)
        dev = {k: to_device(v) for k, v in host.items()}

        @staticmethod
        def out(n, device):
            return torch.full((n,), 0x55, dtype=torch.uint8, device="cuda:0") if device else np.full(n, 0x55, dtype=np.uint8)

        @staticmethod
        def ptr(a):
            return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
    return B


def faults(cases):
    """what was changed and what was said, without the values"""
    return {(message, tuple(sorted(changes))) for message, changes in cases}


def both(block):
    return [(True, block.dev), (False, block.host)]


@pytest.mark.parametrize("kind", ["plain", "cov", "sequences"])
def test_smooth(block, kind):
    said = {}
    for device, src in both(block):
        out, res, cov = block.out(N * 160, device), block.out(64 * (2 if kind == "sequences" else 1), device), block.out(N * 304, device)
        base = dict(d=block.h, obs=block.ptr(src["obs"]), n_frames=N, max_tags=MT, map=block.ptr(src["map"]), n_ids=NI, K=dptr(K), dist=None,
                    n_dist=0, tag_size=0.1, seed=block.ptr(src["seed"]), sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=2,
                    out=block.ptr(out), result=block.ptr(res))
        names = "d obs n_frames max_tags map n_ids K dist n_dist tag_size seed sigma_px sigma_rot sigma_trans max_iters out result"
        entry = {"plain": "asl_smooth_%s", "cov": "asl_smooth_cov_%s", "sequences": "asl_smooth_sequences_%s"}[kind]
        entry %= ("frames_device" if kind != "sequences" else "device") if device else "batch"
        if kind != "plain":
            base["cov"] = block.ptr(cov)
            names += " cov"
        if kind == "sequences":
            base.update(seq_start=offsets(0, 1, N), n_seq=2)
            names = names.replace(" seed ", " seed seq_start n_seq ")
        if device:
            base["stream"] = None
            names += " stream"
        form = Form(entry, names, base, [out, res, cov])
        frames = "n_frames must be in [1, %d] (got 0)" % (1048576 if kind == "sequences" else 65535)
        single = [(NULL_D, dict(d=None)), (NULL_ARG, dict(obs=None)), (NULL_ARG, dict(map=None)), (NULL_ARG, dict(K=None)),
                  (NULL_ARG, dict(out=None)), (NULL_ARG, dict(result=None)), (frames, dict(n_frames=0)),
                  (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4)),
                  (TAG_SIZE, dict(tag_size=0.0)), ("K is not finite", dict(K=dptr(KNAN))), (SIGMAS, dict(sigma_px=0.0)),
                  (SIGMAS, dict(sigma_rot=0.0)), (SIGMAS, dict(sigma_trans=0.0)), (SMOOTH_ITERS % 101, dict(max_iters=101))]
        pairs = [(MAX_TAGS % 0, dict(max_tags=0, sigma_px=0.0)), (N_IDS, dict(n_ids=0, tag_size=0.0)),
                 ("K is not finite", dict(K=dptr(KNAN), max_iters=0))]
        if kind == "cov":
            single += [(NULL_ARG, dict(cov=None))]
            pairs += [(SMOOTH_ITERS % 0, dict(cov=None, max_iters=0))]
        if kind == "sequences":
            run_to = "seq_start must run from 0 to n_frames (got %d to %d, n_frames 2)"
            single += [(NULL_ARG, dict(seq_start=None)), ("n_seq must be in [1, 65535] (got 0)", dict(n_seq=0)),
                       (run_to % (1, 2), dict(seq_start=offsets(1, 1, N))), (run_to % (0, 3), dict(seq_start=offsets(0, 1, 3))),
                       ("sequence 0 must have 1 to 65535 frames (got 0)", dict(seq_start=offsets(0, 0, N))),
                       ("sequence 1 must have 1 to 65535 frames (got -1)", dict(seq_start=offsets(0, 3, N)))]
            pairs += [(run_to % (1, 2), dict(seq_start=offsets(1, 1, N), max_tags=0)), ("n_seq must be in [1, 65535] (got 0)", dict(n_seq=0, n_ids=0))]
        if device:
            single += [(NULL_ARG, dict(seed=None)), ("d_out overlaps d_seed", dict(out=base["seed"])),
                       ("d_out overlaps d_seed", dict(out=base["seed"] + 160 * (N - 1)))]
            pairs += [(SMOOTH_ITERS % 0, dict(seed=None, max_iters=0))]
            if kind != "plain":
                single += [("d_cov overlaps d_out or d_seed", dict(cov=base["out"])), ("d_cov overlaps d_out or d_seed", dict(cov=base["seed"]))]
            if kind == "cov":
                pairs += [(NULL_ARG, dict(cov=None, out=base["seed"]))]
            if kind == "sequences":    # cov NULL is the plain call there: the first overlap speaks
                pairs += [("d_out overlaps d_seed", dict(out=base["seed"], cov=base["seed"]))]
        run(form, single, pairs)
        said[device] = faults(single + pairs)
    assert said[False] <= said[True] and len(said[False]) >= 20    # every fault of the host form, with the device form's message


def test_map(block):
    said = {}
    for device, src in both(block):
        tmap, std, poses, res = block.out(NI * 104, device), block.out(NI * 48, device), block.out(N * 160, device), block.out(64, device)
        base = dict(d=block.h, obs=block.ptr(src["obs"]), n_frames=N, max_tags=MT, n_ids=NI, K=dptr(K), dist=None, n_dist=0, tag_size=0.1,
                    world_id=-1, max_iters=2, map=block.ptr(tmap), tag_std=block.ptr(std), poses=block.ptr(poses), result=block.ptr(res))
        names = "d obs n_frames max_tags n_ids K dist n_dist tag_size world_id max_iters map tag_std poses result"
        if device:
            base["stream"] = None
            names += " stream"
        form = Form("asl_map_frames_device" if device else "asl_map_batch", names, base, [tmap, std, poses, res])
        world, iters = "world_id must be -1 or in [0, n_ids) (got %d)", "max_iters must be in [1, 1000] (got %d)"
        single = [(NULL_D, dict(d=None)), (NULL_ARG, dict(obs=None)), (NULL_ARG, dict(K=None)), (NULL_ARG, dict(map=None)),
                  (NULL_ARG, dict(poses=None)), (NULL_ARG, dict(result=None)), ("n_frames must be >= 1 (got 0)", dict(n_frames=0)),
                  (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4)),
                  (TAG_SIZE, dict(tag_size=0.0)), (world % 1, dict(world_id=1)), (world % -2, dict(world_id=-2)),
                  (iters % 1001, dict(max_iters=1001)), (iters % 0, dict(max_iters=0))]
        pairs = [("n_frames must be >= 1 (got 0)", dict(n_frames=0, max_tags=0)), (MAX_TAGS % 0, dict(max_tags=0, world_id=1)),
                 (world % 1, dict(world_id=1, max_iters=0)), (NULL_D, dict(d=None, obs=None))]
        run(form, single, pairs)
        said[device] = faults(single + pairs)
    assert said[True] == said[False]


def test_calibrate(block):
    said = {}
    for device, src in both(block):
        res, poses = block.out(CALIB_RESULT_DTYPE.itemsize, device), block.out(N * 160, device)
        base = dict(d=block.h, obs=block.ptr(src["obs"]), n_frames=N, max_tags=MT, map=block.ptr(src["map"]), n_ids=NI, tag_size=0.1, width=640,
                    height=480, K_init=None, n_dist=4, flags=0, max_iters=1, result=block.ptr(res), poses=block.ptr(poses))
        names = "d obs n_frames max_tags map n_ids tag_size width height K_init n_dist flags max_iters result poses"
        if device:
            base["stream"] = None
            names += " stream"
        form = Form("asl_calibrate_frames_device" if device else "asl_calibrate_batch", names, base, [res, poses])
        size, k_init = "width and height must be positive (got %d x %d)", "K_init must have finite, positive focal lengths"
        single = [(NULL_D, dict(d=None)), (NULL_ARG, dict(obs=None)), (NULL_ARG, dict(map=None)), (NULL_ARG, dict(result=None)),
                  (NULL_ARG, dict(poses=None)), ("n_frames must be >= 1 (got 0)", dict(n_frames=0)), (MAX_TAGS % 257, dict(max_tags=257)),
                  (N_IDS, dict(n_ids=0)), (N_DIST, dict(n_dist=3)), (TAG_SIZE, dict(tag_size=0.0)), (size % (0, 480), dict(width=0)),
                  (size % (640, -1), dict(height=-1)), ("max_iters must be >= 1 (got 0)", dict(max_iters=0)),
                  ("unknown calibration flags 0x8", dict(flags=8)), (k_init, dict(K_init=dptr(KNAN))), (k_init, dict(K_init=dptr(-K)))]
        pairs = [(size % (0, 480), dict(width=0, flags=8)), ("max_iters must be >= 1 (got 0)", dict(max_iters=0, flags=8)),
                 (TAG_SIZE, dict(tag_size=0.0, width=0)), ("unknown calibration flags 0x8", dict(flags=8, K_init=dptr(KNAN)))]
        run(form, single, pairs)
        said[device] = faults(single + pairs)
    assert said[True] == said[False]


def test_pose_cov(block):
    """asl_pose_cov_device on the block's records, asl_solve_pnp_cov_batch on corners and poses: the same checks"""
    cov_d, cov_h = block.out(N * 304, True), block.out(N * 304, False)
    T = np.tile(np.eye(4), (N, 1, 1))
    T[:, 2, 3] = 1.0
    corners = np.tile(np.array([280, 280, 360, 280, 360, 200, 280, 200], dtype=np.float32), (N, 1))    # a 0.1 tag, 1 in front of K
    KEEP.extend([corners, T])
    cam = dict(K=dptr(K), dist=None, n_dist=0, tag_size=0.1, sigma_px=0.0)
    dev = Form("asl_pose_cov_device", "d obs n K dist n_dist tag_size sigma_px cov stream",
               dict(cam, d=block.h, obs=block.dev["obs"].data_ptr(), n=N, cov=cov_d.data_ptr(), stream=None), [cov_d])
    host = Form("asl_solve_pnp_cov_batch", "d obs T K dist n_dist tag_size sigma_px cov n",
                dict(cam, d=block.h, obs=corners.ctypes.data_as(C.POINTER(C.c_float)), T=T.ctypes.data_as(DP), cov=cov_h.ctypes.data, n=N), [cov_h])
    single = [(NULL_D, dict(d=None)), (NULL_ARG, dict(obs=None)), (NULL_ARG, dict(K=None)), (NULL_ARG, dict(cov=None)),
              ("record count < 0", dict(n=-1)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4)), (TAG_SIZE, dict(tag_size=0.0)),
              (SIGMA_PX, dict(sigma_px=-1.0))]
    pairs = [("record count < 0", dict(n=-1, tag_size=0.0)), (TAG_SIZE, dict(tag_size=0.0, sigma_px=-1.0)), (NULL_D, dict(d=None, K=None)),
             (NO_DIST, dict(n_dist=4, sigma_px=-1.0))]
    run(dev, single, pairs)
    run(host, single + [(NULL_ARG, dict(T=None))], pairs + [(NULL_D, dict(d=None, T=None))])


def test_localize_and_rig(block):
    """asl_localize_cov_frames_device and asl_localize_rig_batch: a covariance form asks for cov before anything else, a rig's
    table is looked at last"""
    out, cov = block.out(N * 160, True), block.out(N * 304, True)
    dev = block.dev
    loc = Form("asl_localize_cov_frames_device", "d obs n_frames max_tags map n_ids K dist n_dist tag_size gate sigma_px out cov stream",
               dict(d=block.h, obs=dev["obs"].data_ptr(), n_frames=N, max_tags=MT, map=dev["map"].data_ptr(), n_ids=NI, K=dptr(K), dist=None, n_dist=0,
                    tag_size=0.1, gate=0.0, sigma_px=0.0, out=out.data_ptr(), cov=cov.data_ptr(), stream=None), [out, cov])
    gate = "max_tag_rms_px must be >= 0 (got -1)"
    run(loc, [(NULL_ARG, dict(cov=None)), (NULL_D, dict(d=None)), (NULL_ARG, dict(K=None)), (NULL_ARG, dict(out=None)), ("n_frames < 0", dict(n_frames=-1)),
              (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)), (N_DIST, dict(n_dist=3, dist=dptr(DIST))), (NO_DIST, dict(n_dist=4)),
              (TAG_SIZE, dict(tag_size=0.0)), (gate, dict(gate=-1.0)), (SIGMA_PX, dict(sigma_px=-1.0))],
        [(NULL_ARG, dict(cov=None, d=None)), (NULL_D, dict(d=None, obs=None)), (MAX_TAGS % 0, dict(max_tags=0, gate=-1.0)),
         (gate, dict(gate=-1.0, sigma_px=-1.0)), ("n_frames < 0", dict(n_frames=-1, n_ids=0))])

    h = block.host
    out = block.out(N * 160, False)
    rig = Form("asl_localize_rig_batch", "d obs n_cams n_frames max_tags map n_ids rig tag_size gate out",
               dict(d=block.h, obs=h["obs"].ctypes.data, n_cams=1, n_frames=N, max_tags=MT, map=h["map"].ctypes.data, n_ids=NI, rig=h["rig"].ctypes.data,
                    tag_size=0.1, gate=0.0, out=out.ctypes.data), [out])

    def table(**fields):
        t = h["rig"].copy()
        for k, v in fields.items():
            t[k] = v
        KEEP.append(t)
        return t.ctypes.data
    cams, slots = "n_cams must be in [1, 16] (got %d)", "n_cams * max_tags must be <= 256 (got 2 x 129)"
    run(rig, [(NULL_D, dict(d=None)), (NULL_ARG, dict(rig=None)), (NULL_ARG, dict(map=None)), ("n_frames < 0", dict(n_frames=-1)),
              (cams % 17, dict(n_cams=17)), (MAX_TAGS % 257, dict(max_tags=257)), (N_IDS, dict(n_ids=0)), (TAG_SIZE, dict(tag_size=0.0)),
              (gate, dict(gate=-1.0)), ("camera 0: n_dist must be 0, 4 or 5 (got 3)", dict(rig=table(n_dist=3))),
              ("camera 0: K is not finite", dict(rig=table(K=KNAN))), ("camera 0: E is not finite", dict(rig=table(E=np.full((3, 4), np.inf))))],
        [(cams % 17, dict(n_cams=17, max_tags=0)), (MAX_TAGS % 0, dict(max_tags=0, rig=table(K=KNAN))), (slots, dict(n_cams=2, max_tags=129, gate=-1.0)),
         (gate, dict(gate=-1.0, rig=table(n_dist=3))), ("camera 0: n_dist must be 0, 4 or 5 (got 3)", dict(rig=table(n_dist=3, K=KNAN)))])


# ---- the pose-graph back-end: asl_gn_solve and its two diagnostics (csrc/gn_host.inc, debug_host.inc) -----------------------

def gn_problem_args():
    """a small good problem (2 tags, 6 cameras) as asl_gn_solve's arguments, and fresh copies of the arrays it may write"""
    from gn_cases import problem_case
    c = problem_case(2, 0, 1e-3)
    oc, ot = np.ascontiguousarray(c["obs_cam"], dtype=np.int32), np.ascontiguousarray(c["obs_tag"], dtype=np.int32)
    KEEP.extend([oc, ot])
    base = dict(d=None, n_cams=len(c["cam0"]), n_tags=2, n_obs=len(oc), obs_cam=oc.ctypes.data_as(IP), obs_tag=ot.ctypes.data_as(IP),
                corners=dptr(c["obs_corners"].reshape(-1, 8)), K=dptr(c["K"]), tag_size=10.0, fixed_tag=0)
    return c, oc, ot, base


GN_EMPTY, GN_FIXED = "empty problem", "fixed_tag out of range"
GN_TAGS = "more than 1000 tags: the dense reduced system is not meant for that"


def gn_list_faults(oc, ot, n_cams):
    """observation lists with one fault each: a camera or a tag out of range on either side, a (camera, tag) pair twice"""
    def ints(a, i, v):
        a = a.copy()
        a[i] = v
        KEEP.append(a)
        return a.ctypes.data_as(IP)
    ref = "observation %d references camera %d / tag %d"
    twice = ot.copy()
    first = int(np.flatnonzero(oc == oc[0])[1])    # camera oc[0]'s second observation: make it its first tag again
    return [(ref % (1, n_cams, ot[1]), dict(obs_cam=ints(oc, 1, n_cams))), (ref % (0, -1, ot[0]), dict(obs_cam=ints(oc, 0, -1))),
            (ref % (2, oc[2], 2), dict(obs_tag=ints(ot, 2, 2))), (ref % (2, oc[2], -1), dict(obs_tag=ints(ot, 2, -1))),
            ("camera %d observes tag %d twice" % (oc[0], ot[0]), dict(obs_tag=ints(twice, first, ot[0])))]


def test_gn_solve(block):
    """every ASL_EINVAL of asl_gn_solve, each followed by a good call on the same detector that still succeeds; the refusal of a
    reduced system that is not positive definite (here: a focal length that is not a number) comes after the solve and leaves
    the poses as they were"""
    c, oc, ot, base = gn_problem_args()
    cam_T, tag_T, stats = np.array(c["cam0"]), np.array(c["tag0"]), np.zeros(3)
    base.update(d=block.h, cam_T=cam_T.ctypes.data_as(DP), tag_T=tag_T.ctypes.data_as(DP), iters=2, stats=stats.ctypes.data_as(DP))
    form = Form("asl_gn_solve", "d n_cams n_tags n_obs obs_cam obs_tag corners K tag_size fixed_tag cam_T tag_T iters stats", base,
                [cam_T, tag_T, stats])
    single = [(NULL_ARG, dict(d=None)), (NULL_ARG, dict(obs_cam=None)), (NULL_ARG, dict(obs_tag=None)), (NULL_ARG, dict(corners=None)),
              (NULL_ARG, dict(K=None)), (NULL_ARG, dict(cam_T=None)), (NULL_ARG, dict(tag_T=None)),
              (GN_EMPTY, dict(n_cams=0)), (GN_EMPTY, dict(n_tags=0)), (GN_EMPTY, dict(n_obs=0)), ("iters must be >= 0 (got -1)", dict(iters=-1)),
              (GN_FIXED, dict(fixed_tag=-1)), (GN_FIXED, dict(fixed_tag=2)), (GN_TAGS, dict(n_tags=1001))] + gn_list_faults(oc, ot, base["n_cams"])
    pairs = [(NULL_ARG, dict(K=None, n_obs=0)), (GN_EMPTY, dict(n_obs=0, fixed_tag=5)), (GN_FIXED, dict(fixed_tag=5, iters=-1)),
             (GN_TAGS, dict(n_tags=1001, iters=-1))]

    def good():
        cam_T[:], tag_T[:] = c["cam0"], c["tag0"]
        assert form() == 0, _lib.load().asl_last_error()
        assert stats[1] < stats[0] and stats[2] >= 1
        return cam_T.copy(), tag_T.copy(), stats.copy()
    first = good()
    for message, changes in single + pairs:
        form.fill()
        form.refuses(message, **changes)
        assert form.untouched(), (message, changes)
        again = good()
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), (message, changes)
    # not positive definite: with a focal length that is not a number the factorisation meets a pivot that is not one either;
    # no trial is accepted and the poses come back as they were
    cam_T[:], tag_T[:] = c["cam0"], c["tag0"]
    form.refuses("reduced system not positive definite (under-constrained problem?)", K=dptr(KNAN))
    assert stats[2] == 0 and np.array_equal(tag_T, c["tag0"]) and np.abs(cam_T - c["cam0"]).max() <= 1e-12
    good()


def test_debug_gn_cholesky(block):
    from gn_cases import dense_case
    c = dense_case(2)
    n, A, b = c["n"], c["A"], c["b"]
    L, y, x, var, Linv, flag = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((1, 48, 48)), np.zeros(1, dtype=np.int32)
    outs = [L, y, x, var, Linv, flag]
    base = dict(d=block.h, A=dptr(A), b=dptr(b), n=n, L=L.ctypes.data_as(DP), n_L=L.size, y=y.ctypes.data_as(DP), x=x.ctypes.data_as(DP),
                var=var.ctypes.data_as(DP), n_vec=n, Linv=Linv.ctypes.data_as(DP), n_Linv=Linv.size, flag=flag.ctypes.data_as(IP))
    form = Form("asl_debug_gn_cholesky", "d A b n L n_L y x var n_vec Linv n_Linv flag", base, outs)
    size = "n must be 6 times a tag count in [1, 1000] (got %d)"
    single = [(NULL_ARG, {k: None}) for k in ("d", "A", "b", "L", "y", "x", "var", "Linv", "flag")]
    single += [(size % 13, dict(n=13)), (size % 0, dict(n=0)), (size % -6, dict(n=-6)), (size % 6006, dict(n=6006)),
               ("L too small: need 144 values (got 143)", dict(n_L=143)), ("y, x and var too small: need 12 values each (got 11)", dict(n_vec=11)),
               ("Linv too small: need 2304 values (got 2303)", dict(n_Linv=2303)),
               ("Linv too small: need 4608 values (got 2304)", dict(n=54, n_L=54 * 54, n_vec=54))]    # a second block needs its own room
    pairs = [(NULL_ARG, dict(A=None, n=13)), (size % 13, dict(n=13, n_L=0)), ("L too small: need 144 values (got 0)", dict(n_L=0, n_vec=0))]
    run(form, single, pairs)
    assert form() == 0 and flag[0] == 0 and np.abs(L @ L.T - A).max() <= 1e-12 * np.abs(A).max()


def test_debug_gn_step(block):
    c, oc, ot, base = gn_problem_args()
    P, M = base["n_cams"], len(oc)
    shapes = _lib.gn_step_shapes(P, 2, M)
    bufs = {k: np.zeros(shapes[k]) for k in _lib.GN_STEP_ITEMS}
    flag = np.zeros(1, dtype=np.int32)

    def spans(short=None, skip=()):
        s = (_lib.DebugSpan * len(_lib.GN_STEP_ITEMS))()
        for i, k in enumerate(_lib.GN_STEP_ITEMS):
            if k not in skip:
                s[i].p, s[i].n = bufs[k].ctypes.data_as(DP), bufs[k].size - (1 if k == short else 0)
        KEEP.append(s)
        return s
    base.update(d=block.h, cam_T=dptr(c["cam0"]), tag_T=dptr(c["tag0"]), lam=1e-3, out=spans(), n_out=len(_lib.GN_STEP_ITEMS),
                flag=flag.ctypes.data_as(IP))
    form = Form("asl_debug_gn_step", "d n_cams n_tags n_obs obs_cam obs_tag corners K tag_size fixed_tag cam_T tag_T lam out n_out flag", base,
                list(bufs.values()) + [flag])
    lam = "lambda must be >= 0 and finite (got %s)"
    single = [(NULL_ARG, {k: None}) for k in ("d", "obs_cam", "obs_tag", "corners", "K", "cam_T", "tag_T", "out")]
    single += [(GN_EMPTY, dict(n_cams=0)), (GN_EMPTY, dict(n_tags=0)), (GN_EMPTY, dict(n_obs=0)), (GN_FIXED, dict(fixed_tag=-1)),
               (GN_FIXED, dict(fixed_tag=2)), (GN_TAGS, dict(n_tags=1001)), (lam % "-1", dict(lam=-1.0)), (lam % "nan", dict(lam=float("nan"))),
               (lam % "inf", dict(lam=float("inf"))), ("out must have 11 entries (got 10)", dict(n_out=10))] + gn_list_faults(oc, ot, P)
    need = dict(zip(_lib.GN_STEP_ITEMS, (156 * M, M, 1, 36 * P, 6 * P, 36 * M, 144, 12, 12, 12 * P, 24)))
    single += [("out[%d] too small: need %d values (got %d)" % (i, need[k], need[k] - 1), dict(out=spans(short=k))) for i, k in enumerate(_lib.GN_STEP_ITEMS)]
    pairs = [(GN_EMPTY, dict(n_obs=0, lam=-1.0)), (lam % "-1", dict(lam=-1.0, n_out=3)), ("out must have 11 entries (got 3)", dict(n_out=3, out=spans(short="S")))]
    run(form, single, pairs)
    # the flag and every item are optional
    assert form(flag=None, out=spans(skip=_lib.GN_STEP_ITEMS)) == 0 and form.untouched()
    assert form() == 0 and flag[0] == 0 and bufs["dG"][1].any() and not bufs["dG"][0].any()
