"""Inputs and recorded bounds of the rig sequence-localisation tests (tests/test_smooth_rig_ref.py on the CPU,
tests/test_gpu_smooth_rig.py on the device), built with rig_cases.exact_block / mounting and the smooth_cases helpers, seeded
by rig_ref.localize.  Every figure in recorded() and DEVICE_TOL was measured on the CPU with the NumPy statement
(tests/smooth_ref.py) -- never with the kernels; test_smooth_rig_ref.py measures them again and requires the recorded
figures to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import localize_cases as LC
import rig_cases as RC
import rig_ref as RR
import smooth_cases as SC
import smooth_ref as SR
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

TAG = LC.TAG_INNER
MAX_ITERS = SC.MAX_ITERS
COMPARE_ITERS = SC.COMPARE_ITERS          # for the reason given in smooth_cases: the converged tail's trial count is rounding
SHAPE_SIGMAS = SC.SHAPE_SIGMAS
HOLES_SIGMAS, FLIPS_SIGMAS, NOISE_SIGMAS = SC.HOLES_SIGMAS, SC.FLIPS_SIGMAS, SC.NOISE_SIGMAS
NOISE_SEED, NOISE_PX = 11, 0.3
HUBER_PX = 1.0

# Bound of the device's T against the statement's, by the project's rule (smooth_cases.DEVICE_TOL): ten times the largest
# rel_err between the statement and the statement with every frame's corner sums accumulated in reversed slot order (a pure
# rounding perturbation) over all the cases of this file (all_cases(), plain and at HUBER_PX), floor 1e-9.  Every case is
# measured at COMPARE_ITERS trials (reversal_error), the trials at which the device is compared with the statement: at
# MAX_ITERS the reversed statement of noise() runs 30 trials where the statement runs 6 and its poses end 1.6e-7 apart, the
# converged tail smooth_cases describes -- a property of the stop rule, not of the arithmetic this bound is for.
# Measured: 6.13e-14 at outliers() with HUBER_PX; no_posed and flip 0 (nothing to solve; one slot has no order to reverse).
DEVICE_TOL_MEASURED = 6.13e-14
DEVICE_TOL = max(10 * DEVICE_TOL_MEASURED, 1e-9)


def recorded():
    """the statement's figures, rounded up to 4 significant digits; expected values next to each
    holes_end_err / holes_mid_err: position error against the truth of the emptied frames 0 and 6 / of frame 3 of holes()
      (scene units).  As for one camera: a random walk holds an end frame at its neighbour, one frame step (0.3 units) from
      the truth, and puts frame 3 half way between its neighbours, where the straight trajectory has it (expected: 0.3 and
      float32-corner noise, about 1e-5).
    flip_margin: the largest final rotation error of the re-mirrored frames of flip() over the largest rotation error of the
      unmirrored frames' seeds (expected: of the order of smooth_cases' flips_margin, 10.59; the mirrored seeds themselves
      are some thousand times the unmirrored seeds' error off).
    noise_rmse_frame / noise_rmse_smooth: position RMSE against the truth of the per-frame rig localisation / of the
      statement on noise() (scene units; expected: smoothed a fraction of per-frame, as 0.1381 against 0.4276 for one camera).
    outlier_rmse_plain / outlier_rmse_huber: the same of the statement on outliers() without and with HUBER_PX (expected: the
      Huber figure near noise_rmse_smooth, the plain one above it.  Measured: the plain solve is 10.19 units off -- the slot
      with another tag's corners throws its frame's seed far out, and the squared loss drags the neighbours after it -- the
      Huber solve 0.1872, next to 0.1181 without the two outliers)."""
    return {"holes_end_err": 0.3001, "holes_mid_err": 2.950e-5, "flip_margin": 16.46, "noise_rmse_frame": 0.6280, "noise_rmse_smooth": 0.1181,
            "outlier_rmse_plain": 10.19, "outlier_rmse_huber": 0.1872}


PAIR = Rig([RigCamera(RC.K45, None, RC.mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(RC.K45, None, RC.mounting(7.0, (4.0, 0.5, 0.0), 2.0))])


def ring(n_cams):
    """n_cams cameras fanned over 28 degrees of yaw and 14 units of offset, as rig_cases' ring of 8"""
    if n_cams == 2:
        return PAIR
    step = 1.0 / (n_cams - 1)
    return Rig([RigCamera(RC.K45, None, RC.mounting(-14.0 + 28.0 * step * c, (-7.0 + 14.0 * step * c, 0.3 * (c % 3), 0.0), 1.0 * (c % 2)))
                for c in range(n_cams)])


def rig_poses(n, per_round=520):
    """world<-rig along the bench trajectory"""
    return [LC.world_from_camera(p, r) for p, r in LC.trajectory(per_round)[:n]]


def empty(obs, frames, cams=None):
    """the frames' records emptied in the given cameras (None: in all of them)"""
    out = obs.copy()
    for c in range(obs.shape[0]) if cams is None else cams:
        for f in frames:
            out["flags"][c, f] = 0
            out["id"][c, f] = -1
    return out


def noisy(obs, px, seed):
    return SC.noisy(obs, px, seed)


def seeds_of(obs, rec, rig):
    """the per-frame rig localisation of the block: what asl_localize_rig_frames_device writes for it"""
    return RR.localize(obs, rec, rig, TAG)


def mirror_seed(obs, rec, rig, seed, frames, sigmas):
    """the seeds of `frames` replaced by candidate B of the chain: their mirrored planar minima through the mounting"""
    out = seed.copy()
    cand = SR.candidates(SR.rig_problem(obs, rec, rig, TAG, *sigmas), seed)
    for f in frames:
        assert cand[f][2]
        R, t = cand[f][1]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
        out["T"][f] = T
    return out


def scene():
    tm = TagMap.from_scene(LC.bench_scene())
    return tm, tm.as_records()


# (n_cams, max_tags, n_frames): division magic at max_tags 1 and at a non-power of two; 15 slots = 60 corners, which do not
# fill a wavefront round; 256 slots = the full 1024 corners and the full LDS (also (8, 32): rig_cases "slots_256", below);
# n_frames 1, 2, 64 and 65: the dynamic programme and the scan carry state across a 64-frame load
SHAPES = [(2, 1, 65), (2, 3, 2), (3, 5, 64), (16, 16, 1)]


@functools.lru_cache(maxsize=None)
def shape(n_cams, max_tags, n):
    """(obs, map records, rig, seeds): n consecutive frames of the bench trajectory at 520 frames a round, corners with 0.2 px
    noise, seeded by the rig localisation of the same frames without the noise (so that the first trials have work to do);
    every 7th frame from the 4th on emptied in every camera (n >= 5)"""
    tm, rec = scene()
    rig = ring(n_cams)
    exact = RC.exact_block(tm, rig, rig_poses(n), TAG, max_tags)
    obs = noisy(exact, 0.2, 1000 * n_cams + 10 * max_tags + n)
    if n >= 5:
        obs, exact = empty(obs, range(3, n, 7)), empty(exact, range(3, n, 7))
    return obs, rec, rig, seeds_of(exact, rec, rig)


@functools.lru_cache(maxsize=None)
def from_rig_cases(name):
    """(obs, map records, rig, seeds) of a rig_cases case ("slots_256": 8 x 32; "mixed_models": a 5-coefficient lens next to a
    pinhole of another focal length), corners with 0.2 px noise, seeded from the exact block"""
    c = RC.case(name)
    return noisy(c["obs"], 0.2, 77), c["rec"], c["rig"], seeds_of(c["obs"], c["rec"], c["rig"])


@functools.lru_cache(maxsize=None)
def holes():
    """(obs, map records, rig, seeds, truths): exact corners on a straight, rotation-free trajectory of 7 frames, 4 tags a
    camera; frames 0, 3 and 6 (start, middle, end) emptied in every camera, camera 1 with nothing in frames 1 to 4"""
    tm, rec = scene()
    poses = [LC.world_from_camera((-0.9 + 0.3 * i, 0.2, 0.5), (0.0, 0.0, 0.0)) for i in range(7)]
    obs = empty(empty(RC.exact_block(tm, PAIR, poses, TAG, 4), (0, 3, 6)), range(1, 5), cams=(1,))
    return obs, rec, PAIR, seeds_of(obs, rec, PAIR), np.array(poses)


FLIP_FRAMES = (3, 4, 9)


@functools.lru_cache(maxsize=None)
def flip():
    """(obs, map records, rig, seeds, truths, mirrored frames): 12 frames of smooth_cases' one small, near-frontal tag, seen by
    camera 1 alone (camera 0's records emptied), whose mounting is turned and offset; the seeds of FLIP_FRAMES replaced by
    their mirrored minima, so that the chain's B has to come back through inv(E_1)"""
    tm = TagMap.from_scene(SC.FLIP_TAG)
    rec = tm.as_records()
    poses = [LC.world_from_camera((-3.0 + 0.5 * i, 1.0 + 0.2 * i, 0.3 * i), (2.0 + 0.1 * i, -3.0 + 0.15 * i, 0.2 * i)) for i in range(12)]
    obs = empty(RC.exact_block(tm, PAIR, poses, TAG, 1, pnp_seed=None), range(12), cams=(0,))
    assert (obs["flags"][1, :, 0] & 1).all()
    seed = seeds_of(obs, rec, PAIR)
    return obs, rec, PAIR, mirror_seed(obs, rec, PAIR, seed, FLIP_FRAMES, FLIPS_SIGMAS), np.array(poses), FLIP_FRAMES


@functools.lru_cache(maxsize=None)
def noise():
    """(obs, map records, rig, seeds, truths): 40 consecutive frames of the bench trajectory at 400 frames a round, two tags a
    camera, float32 corners plus Gaussian noise of NOISE_PX from NOISE_SEED"""
    tm, rec = scene()
    poses = rig_poses(40, 400)
    obs = noisy(RC.exact_block(tm, PAIR, poses, TAG, 2), NOISE_PX, NOISE_SEED)
    return obs, rec, PAIR, seeds_of(obs, rec, PAIR), np.array(poses)


OUTLIER_SLIP = (1, 12, 0)      # (camera, frame, slot): corner 2 moved by 8 px
OUTLIER_SWAP = (1, 27, 1)      # carries the corners of slot 0 of its frame and camera


@functools.lru_cache(maxsize=None)
def outliers():
    """noise() with one slipped corner and one slot carrying another tag's corners, both in camera 1; seeded by the rig
    localisation of the corrupted block"""
    obs, rec, rig, _, truth = noise()
    obs = obs.copy()
    c, f, s = OUTLIER_SLIP
    obs["corners"][c, f, s].reshape(4, 2)[2] += np.array([8.0, -3.0], dtype=np.float32)
    c, f, s = OUTLIER_SWAP
    obs["corners"][c, f, s] = obs["corners"][c, f, 0]
    assert (obs["flags"][1, (12, 27)] & 1).all()
    return obs, rec, rig, seeds_of(obs, rec, rig), truth


@functools.lru_cache(maxsize=None)
def no_posed():
    """(obs, map records, rig, seeds): no frame has a tag in any camera: result status 1"""
    obs, rec, rig, _ = shape(2, 3, 2)
    obs = empty(obs, range(2))
    return obs, rec, rig, seeds_of(obs, rec, rig)


SEQ_START = np.array([0, 1, 3, 68], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def three_sequences():
    """(obs, map records, rig, seeds): 68 frames cut into sequences of 1, 2 and 65 frames (SEQ_START)"""
    return shape(2, 3, 68)


GAP_FRAMES = 9


@functools.lru_cache(maxsize=None)
def gap():
    """(obs, map records, rig, seeds, times): GAP_FRAMES frames of shape (3, 5), frames 4 to 8 five time units late"""
    times = np.arange(GAP_FRAMES, dtype=np.float64)
    times[4:] += 5.0
    return shape(3, 5, GAP_FRAMES) + (times,)


def all_cases():
    """[(name, obs, map records, rig, seeds, sigmas, max_iters, times)]: every case of this file"""
    out = [("holes",) + holes()[:4] + (HOLES_SIGMAS, MAX_ITERS, None), ("flip",) + flip()[:4] + (FLIPS_SIGMAS, MAX_ITERS, None),
           ("noise",) + noise()[:4] + (NOISE_SIGMAS, MAX_ITERS, None), ("outliers",) + outliers()[:4] + (NOISE_SIGMAS, MAX_ITERS, None)]
    out += [("shape%d_%d_%d" % s,) + shape(*s) + (SHAPE_SIGMAS, COMPARE_ITERS, None) for s in SHAPES]
    out += [(n,) + from_rig_cases(n) + (SHAPE_SIGMAS, COMPARE_ITERS, None) for n in ("slots_256", "mixed_models")]
    out += [("no_posed",) + no_posed() + (SHAPE_SIGMAS, COMPARE_ITERS, None), ("gap",) + gap()[:4] + (SHAPE_SIGMAS, COMPARE_ITERS, gap()[4])]
    return out


COMPARE = ["shape%d_%d_%d" % s for s in SHAPES] + ["slots_256", "mixed_models", "no_posed", "gap"]   # device against statement
SCENES = ["holes", "flip", "noise", "outliers"]                                                         # at full iterations


def case(name):
    return [c for c in all_cases() if c[0] == name][0]


def run(name, reverse=False, huber=0.0, max_iters=None):
    _, obs, rec, rig, seed, sig, iters, times = case(name)
    return SR.smooth_rig(obs, rec, rig, TAG, seed, *sig, max_iters or iters, times=times, reverse=reverse, huber_px=huber)


def reversal_error(name, huber):
    """rel_err of T between the statement and the statement with reversed corner sums, both at COMPARE_ITERS trials"""
    a, b = run(name, huber=huber, max_iters=COMPARE_ITERS), run(name, reverse=True, huber=huber, max_iters=COMPARE_ITERS)
    return LC.rel_err(a[0]["T"], b[0]["T"])


@functools.lru_cache(maxsize=None)
def statement(name, huber=0.0):
    """the statement's (poses, result, trace) of a case of all_cases(), computed once"""
    return run(name, huber=huber)


def pos_rmse(T, truth):
    return float(np.sqrt(np.mean(np.square(SC.pos_err(T, truth)))))


def flip_errors(T):
    """(largest rotation error of the re-mirrored frames of T, largest of the unmirrored frames' seeds)"""
    _, _, _, seed, tr, frames = flip()
    rest = [f for f in range(len(tr)) if f not in frames]
    return (max(LC.rot_err(T[f], tr[f]) for f in frames), max(LC.rot_err(seed["T"][f], tr[f]) for f in rest))


def figures(poses_of):
    """the figures of recorded(), from poses_of(name, huber) -> the (n_frames,) poses of a scene's solve at full iterations"""
    h, n, o = holes()[4], noise()[4], outliers()[4]
    Th = poses_of("holes", 0.0)["T"]
    fl = flip_errors(poses_of("flip", 0.0)["T"])
    return {"holes_end_err": float(SC.pos_err(Th[[0, 6]], h[[0, 6]]).max()), "holes_mid_err": float(SC.pos_err(Th[3], h[3])),
            "flip_margin": fl[0] / fl[1], "noise_rmse_frame": pos_rmse(noise()[3]["T"], n),
            "noise_rmse_smooth": pos_rmse(poses_of("noise", 0.0)["T"], n),
            "outlier_rmse_plain": pos_rmse(poses_of("outliers", 0.0)["T"], o), "outlier_rmse_huber": pos_rmse(poses_of("outliers", HUBER_PX)["T"], o)}
