"""Sequence localisation: the camera poses of one camera's consecutive frames against a known tag map, solved together
under a random-walk motion prior (asl_smooth_batch / asl_smooth_frames_device, k_smooth.inc).  Every frame gets a pose: one
without a mapped tag is carried by its neighbours, a single-tag frame is kept out of its mirrored planar minimum by them,
and corner noise is averaged over the sequence.
Several sequences in one call, solved side by side: Detector.smooth_sequences / TagDetector.localize_sequences
(asl_smooth_sequences_batch), one SmoothResult per sequence.
With huber_px > 0 (asl_smooth_robust_sequences_batch) every corner's pixel residual goes through a Huber loss of that
threshold: a slipped corner or a slot with another tag's corners is down-weighted instead of bending its frame and its
neighbours.  SmoothResult.n_soft counts the slots it down-weighted, .soft marks their frames.

    SmoothResult         the poses (CAM_POSE_DTYPE per frame), the SMOOTH_RESULT_DTYPE record, the filled / flipped / soft masks and,
                         from a solve with with_cov (asl_smooth_cov_batch), every pose's covariance (POSE_COV_DTYPE per frame)
    SMOOTH_RESULT_DTYPE  cost_seed, cost, rms_px, rms_seed_px, n_frames_data, n_filled, n_flipped, iterations, status, n_soft
"""
import numpy as np

from ._lib import CAM_POSE_DTYPE, POSE_COV_DTYPE, SMOOTH_RESULT_DTYPE
from .localize import pose_std

FRAME_DATA, FRAME_NOTHING, FRAME_FAILED, FRAME_PRIOR = 0, 1, 4, 6
STATUS_OK, STATUS_NO_POSED_FRAME, STATUS_NOT_POSITIVE_DEFINITE, STATUS_NON_FINITE = 0, 1, 2, 3
FLIPPED = 256   # added to seed_slot where the seed chain chose the mirrored candidate

__all__ = ["SmoothResult", "SMOOTH_RESULT_DTYPE", "CAM_POSE_DTYPE", "FRAME_DATA", "FRAME_NOTHING", "FRAME_FAILED", "FRAME_PRIOR",
           "STATUS_OK", "STATUS_NO_POSED_FRAME", "STATUS_NOT_POSITIVE_DEFINITE", "STATUS_NON_FINITE", "FLIPPED"]


class SmoothResult:
    """What Detector.smooth returns, named."""

    def __init__(self, poses, result, seed=None, cov=None):
        self.poses = np.asarray(poses, dtype=CAM_POSE_DTYPE)
        self.result = np.asarray(result, dtype=SMOOTH_RESULT_DTYPE).reshape(())
        self.seed = seed    # the per-frame localisation that seeded the solve (None: not kept)
        self.cov_records = None if cov is None else np.asarray(cov, dtype=POSE_COV_DTYPE)   # None: solved without with_cov

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
