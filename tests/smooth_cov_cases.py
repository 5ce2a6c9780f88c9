"""Inputs and recorded figures of the tests of the smoothed poses' covariance (tests/test_smooth_cov_ref.py on the CPU,
tests/test_gpu_smooth_cov.py on the device).  As in smooth_cases.py, every recorded figure was measured on the CPU with the
NumPy statement (tests/smooth_cov_ref.py) -- never with the kernels; test_smooth_cov_ref.py measures them again and requires
them to still hold, so the GPU tests can use them without recomputing."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import pose_cov_ref as PC
import smooth_cases as SC
import smooth_cov_ref as SV
import smooth_ref as SR
from aprilslam_amd import _lib
from aprilslam_amd.localize import TagMap

# the cases of the device-against-statement comparison: one frame (no M), two frames (one coupling), the 64 / 65 boundary
# of the per-lane loads upstream, two and a bit chunks, one slot a frame, lens coefficients, long prior-only runs, data only
# at the first or the last frame
DEVICE_CASES = ["shape1_1_0", "shape1_4_0", "shape2_4_0", "shape3_1_0", "shape5_4_5", "shape64_4_0", "shape65_1_5", "shape65_4_5",
                "shape130_4_0", "holes", "flips", "noise", "hole70", "first_only", "last_only", "one_id"]
NO_SOLVE_CASES = ["all_empty", "behind", "nonfinite"]     # smooth result status 1, 2, 3: covariance status 1


def recorded():
    """the statement's figures, to the digits given (position std = |sqrt(diag C[3:])|, scene units)
    holes_end_std / holes_mid_std: the emptied frames 0 and 6 / frame 3 of smooth_cases.holes().  Analytic, for a neighbour
      without uncertainty: sqrt(3) sigma_trans = 3.4641 for one step of the prior and sqrt(3) sigma_trans / sqrt(2) = 2.4495
      between two; the rest is the neighbours' own uncertainty.  holes_data_std: the range of the four frames with data.
    hole70_peak: (frame, std) of the largest position std of smooth_cases' hole70 (frames 2..71 emptied); hole70_rims: the
      std at frames 1 and 72, the frames with data next to the hole.
    pivot_floor: the smallest pivot over its diagonal entry of D_f over all cases of smooth_cases.all_cases() (flips): far
      above pose_cov_ref.PIVOT_TOL, so none of them is decided by the threshold."""
    return {"holes_end_std": 3.4649, "holes_mid_std": 2.4500, "holes_data_std": (0.0723, 0.0730), "hole70_peak": (36, 1.5019),
            "hole70_rims": (0.5125, 0.4577), "pivot_floor": 2.4e-6}


DIGITS = 5e-5    # half a unit of the last recorded digit


def case(name):
    """(obs, map records, seeds, dist, sigmas, max_iters) of a case of smooth_cases.all_cases() or failure_cases()"""
    if name in SC.failure_cases():
        obs, rec, seed, sig, iters, _, _ = SC.failure_cases()[name]
        return obs, rec, seed, None, sig, iters
    return [c[1:] for c in SC.all_cases() if c[0] == name][0]


@functools.lru_cache(maxsize=None)
def prior_only():
    """(obs, map records, seeds, dist, sigmas, max_iters): frames 1, 2 and 4 of holes() with their seeds kept and their
    observations emptied.  The LM's damping solves it (result status 0, frames status 6); the undamped matrix is a pure
    motion prior, which leaves the six directions of a common motion of all frames free: covariance status 2."""
    obs, rec, seed, _ = SC.holes()
    keep = [1, 2, 4]
    return SC.empty(obs[keep], range(3)), rec, seed[keep].copy(), None, SC.HOLES_SIGMAS, 4


@functools.lru_cache(maxsize=None)
def statement(name):
    """(poses, result) of the statement's smooth for a case name of this file"""
    obs, rec, seed, dist, sig, iters = prior_only() if name == "prior_only" else case(name)
    return SC.run(obs, rec, seed, dist, sig, max_iters=iters)[:2]


@functools.lru_cache(maxsize=None)
def statement_cov(name):
    """the statement's covariance at the statement's own poses"""
    obs, rec, seed, dist, sig, iters = prior_only() if name == "prior_only" else case(name)
    poses, res = statement(name)
    return SV.smooth_cov(obs, rec, SC.K, dist, SC.TAG, poses, res, *sig)[0]


# ---- statistical consistency: sequences drawn from the prior itself

NEES_RUNS, NEES_FRAMES, NEES_EMPTY, NEES_TAGS = 60, 8, 3, 4
NEES_SIGMAS = SC.NOISE_SIGMAS
NEES_BAND = 4.0 * np.sqrt(12.0 / NEES_RUNS)     # a chi-square of 6 dof has variance 12: four sigma of a mean over the runs


def frame_from_pose(rec, R, t, max_tags):
    """localize_cases.exact_frame of a camera<-world pose (R, t): the first max_tags tags of the map, in id order, that lie in
    front of the camera with every corner inside the image, projected exactly"""
    cam = LR.camera(SC.K, None)
    obj = LR.object_corners(SC.TAG)
    obs = np.zeros(max_tags, dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    k = 0
    for i in range(len(rec)):
        M = np.asarray(rec["T"][i], dtype=np.float64).reshape(3, 4)
        Pc = (np.c_[obj, np.zeros(4)] @ M[:, :3].T + M[:, 3]) @ R.T + t
        if k == max_tags or not rec["valid"][i] or np.any(Pc[:, 2] <= 1e-3):
            continue
        uv = LR.project(cam, Pc)
        if np.any(uv < 0) or np.any(uv[:, 0] >= LC.W) or np.any(uv[:, 1] >= LC.H):
            continue
        obs["id"][k], obs["flags"][k], obs["corners"][k] = i, 3, uv.ravel()
        obs["T"][k] = np.c_[R @ M[:, :3], R @ M[:, 3] + t].ravel()
        k += 1
    return obs


def prior_walk(run):
    """(obs, map records, true camera<-world poses) of one run: NEES_FRAMES poses from LC.trajectory(400)[0], each next one
    drawn from the motion prior, P_{f+1} = (Rod(a) R_f, Rod(a) t_f + b), a ~ N(0, sigma_rot^2), b ~ N(0, sigma_trans^2);
    NEES_TAGS tags a frame with N(0, sigma_px^2) corner noise, frame NEES_EMPTY emptied; rng seed 1000 + run"""
    rng = np.random.default_rng(1000 + run)
    spx, srot, strans = NEES_SIGMAS
    rec = TagMap.from_scene(LC.bench_scene()).as_records()
    T0 = np.linalg.inv(LC.world_from_camera(*LC.trajectory(400)[0]))
    P = [(T0[:3, :3], T0[:3, 3])]
    for _ in range(NEES_FRAMES - 1):
        a, b = rng.normal(0.0, srot, 3), rng.normal(0.0, strans, 3)
        dR = LR.rodrigues(a)
        P.append((dR @ P[-1][0], dR @ P[-1][1] + b))
    obs = np.stack([frame_from_pose(rec, R, t, NEES_TAGS) for R, t in P])
    noise = rng.normal(0.0, spx, obs["corners"].shape)
    obs["corners"] = (obs["corners"].astype(np.float64) + noise).astype(np.float32)
    return SC.empty(obs, (NEES_EMPTY,)), rec, P


def nees_of_run(run):
    """(NEES_FRAMES,) e^T C^-1 e of the statement's smooth and covariance against the run's truth"""
    obs, rec, P = prior_walk(run)
    poses, res, _ = SC.run(obs, rec, SC.seeds_of(obs, rec), None, NEES_SIGMAS)
    cov = SV.smooth_cov(obs, rec, SC.K, None, SC.TAG, poses, res, *NEES_SIGMAS)[0]
    assert res["status"] == 0 and (cov["status"] == 0).all()
    out = np.zeros(len(P))
    for f, (R, t) in enumerate(P):
        T = np.asarray(poses["T"][f])
        e = PC.pose_error(T[:3, :3], T[:3, 3], R.T, -(R.T @ t))
        out[f] = e @ np.linalg.solve(cov["cov"][f], e)
    return out
