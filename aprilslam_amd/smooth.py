"""Sequence localisation: the camera poses of one camera's consecutive frames against a known tag map, solved together
under a random-walk motion prior (asl_smooth_batch / asl_smooth_frames_device, k_smooth.inc).  Every frame gets a pose: one
without a mapped tag is carried by its neighbours, a single-tag frame is kept out of its mirrored planar minimum by them,
and corner noise is averaged over the sequence.
Several sequences in one call, solved side by side: Detector.smooth_sequences / TagDetector.localize_sequences
(asl_smooth_sequences_batch), one SmoothResult per sequence.
With huber_px > 0 (asl_smooth_robust_sequences_batch) every corner's pixel residual goes through a Huber loss of that
threshold: a slipped corner or a slot with another tag's corners is down-weighted instead of bending its frame and its
neighbours.  SmoothResult.n_soft counts the slots it down-weighted, .soft marks their frames.
With times (asl_smooth_timed_sequences_batch) every frame has a time, sigma_rot and sigma_trans are the random walk's per
unit of that time, and a pair of frames dt apart is held by the prior / sqrt(dt): dropped frames, a camera pause and a
variable frame rate are one sequence.  SmoothResult.pose_at(t) is the pose between two frames along the prior's geodesic.

    SmoothResult         the poses (CAM_POSE_DTYPE per frame), the SMOOTH_RESULT_DTYPE record, the filled / flipped / soft masks and,
                         from a solve with with_cov (asl_smooth_cov_batch), every pose's covariance (POSE_COV_DTYPE per frame)
    SMOOTH_RESULT_DTYPE  cost_seed, cost, rms_px, rms_seed_px, n_frames_data, n_filled, n_flipped, iterations, status, n_soft
"""
import numpy as np

from ._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE
from .localize import pose_std

FRAME_DATA, FRAME_NOTHING, FRAME_FAILED, FRAME_PRIOR = 0, 1, 4, 6
STATUS_OK, STATUS_NO_POSED_FRAME, STATUS_NOT_POSITIVE_DEFINITE, STATUS_NON_FINITE, STATUS_BAD_TIMES = 0, 1, 2, 3, 4
FLIPPED = 256   # added to seed_slot where the seed chain chose the mirrored candidate

__all__ = ["SmoothResult", "SMOOTH_RESULT_DTYPE", "CAM_POSE_DTYPE", "FRAME_DATA", "FRAME_NOTHING", "FRAME_FAILED", "FRAME_PRIOR",
           "STATUS_OK", "STATUS_NO_POSED_FRAME", "STATUS_NOT_POSITIVE_DEFINITE", "STATUS_NON_FINITE", "STATUS_BAD_TIMES", "FLIPPED"]


def _log_so3(R):
    """the rotation vector of R, as the solve's motion residual takes it (atan2 of |vee| and the trace)"""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt(a @ a)
    return a * (np.arctan2(s, 0.5 * (np.trace(R) - 1.0)) / s) if s > 1e-12 else a


def _exp_so3(w):
    theta = np.sqrt(w @ w)
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    k = w / theta
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(theta) * np.eye(3) + (1.0 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * Kx


class SmoothResult:
    """What Detector.smooth returns, named."""

    def __init__(self, poses, result, seed=None, cov=None, times=None):
        self.poses = np.asarray(poses, dtype=CAM_POSE_DTYPE)
        self.result = np.asarray(result, dtype=SMOOTH_RESULT_DTYPE).reshape(())
        self.seed = seed    # the per-frame localisation that seeded the solve (None: not kept)
        self.cov_records = None if cov is None else np.asarray(cov, dtype=POSE_COV_DTYPE)   # None: solved without with_cov
        self.times = None if times is None else np.array(times, dtype=np.float64).ravel()   # None: frame f is at time f
        if self.times is not None and len(self.times) != len(self.poses):
            raise ValueError("times must hold one value per frame")

    @property
    def ok(self):
        return int(self.result["status"]) == STATUS_OK

    @property
    def filled(self):
        """frames that had no pose of their own (no seed): started from a neighbour's"""
        return (self.poses["seed_slot"] < 0) & (self.poses["status"] != FRAME_NOTHING)

    @property
    def flipped(self):
        """frames where the seed chain took the mirrored planar minimum instead of the seed"""
        if self.seed is None:
            raise ValueError("the flipped mask needs the seed poses the solve started from")
        return (self.poses["seed_slot"] >= 0) & (self.poses["seed_slot"] == np.asarray(self.seed)["seed_slot"] + FLIPPED)

    @property
    def prior_only(self):
        """frames without a mapped tag: their pose comes from the motion prior alone"""
        return self.poses["status"] == FRAME_PRIOR

    @property
    def n_soft(self):
        """taking-part slots, over all frames, with a corner over the Huber threshold at the returned poses (0 from a solve
        without huber_px)"""
        return int(self.result["n_soft"])

    @property
    def soft(self):
        """frames with such a slot (their n_rejected counts them): down-weighted, not removed"""
        return self.poses["n_rejected"] > 0

    def trajectory(self):
        """(n_frames, 4, 4) world<-camera"""
        return np.array(self.poses["T"], dtype=np.float64).reshape(-1, 4, 4)

    def pose_at(self, t):
        """(4, 4) world<-camera at the time t inside the sequence (without times: the frame index), along the prior's own
        geodesic between the two frames around it: with a = (t - times[f]) / (times[f + 1] - times[f]) and (R_D, t_D) the step
        from frame f to f + 1, camera<-world R = Exp(a Log R_D) R_f, t = Exp(a Log R_D) t_f + a t_D -- the random walk's
        conditional mean between the two poses, to first order in the step rotation.  At a frame's own time it is that
        frame's pose.  No extrapolation: a t outside [times[0], times[-1]] is a ValueError, and so is a solve that is not ok."""
        if not self.ok:
            raise ValueError("the solve has no poses (result status %d)" % int(self.result["status"]))
        n = len(self.poses)
        times = np.arange(n, dtype=np.float64) if self.times is None else self.times
        t = float(t)
        if not (times[0] <= t <= times[-1]):
            raise ValueError("t = %r is outside the sequence's times [%r, %r]" % (t, float(times[0]), float(times[-1])))
        T = self.trajectory()
        f = int(np.searchsorted(times, t, side="right")) - 1
        if f == n - 1 or t == times[f]:
            return T[f].copy()
        Ra, Rb = T[f][:3, :3].T, T[f + 1][:3, :3].T
        ta, tb = -(Ra @ T[f][:3, 3]), -(Rb @ T[f + 1][:3, 3])
        a = (t - times[f]) / (times[f + 1] - times[f])
        RD = Rb @ Ra.T
        tD = tb - RD @ ta
        E = _exp_so3(a * _log_so3(RD))
        R, tv = E @ Ra, E @ ta + a * tD
        out = np.eye(4)
        out[:3, :3], out[:3, 3] = R.T, -(R.T @ tv)
        return out

    def _cov_records(self):
        if self.cov_records is None:
            raise ValueError("the solve ran without the covariance: pass with_cov=True")
        return self.cov_records

    @property
    def cov(self):
        """(n_frames, 6, 6) covariance of every frame's world<-camera pose, order (rx ry rz | px py pz) (include/aprilslam.h:
        asl_pose_cov): the frame's marginal under the corner noise and the motion prior of the solve.  Zeros where
        cov_status is not 0."""
        return np.array(self._cov_records()["cov"], dtype=np.float64).reshape(-1, 6, 6)

    @property
    def cov_status(self):
        """per frame, the same in all: 0 ok, 1 the solve has no covariance (it failed or had nothing to solve), 2 the
        information matrix is not positive definite (e.g. no frame of the sequence has a mapped tag)"""
        return np.array(self._cov_records()["status"])

    def pose_std(self):
        """(rotation std in rad (n_frames, 3), position std (n_frames, 3)): localize.pose_std of cov"""
        return pose_std(self.cov)
