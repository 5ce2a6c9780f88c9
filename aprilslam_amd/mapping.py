"""Tag-map reconstruction from a batch of frames (asl_map_batch / asl_map_frames_device).

Frames that see an unknown set of tags give the tags' world<-tag poses (the world tag at the identity), every frame's
camera pose and a per-tag standard deviation; the map is the asl_map_tag block localisation reads (localize.TagMap).

    MapResult           the records of one solve, with .tag_map, .tag_std, .camera_poses, .frame_status and, from a solve
                        with a robust loss (huber_px), .n_soft, .slot_weight and .soft_slots(); from a solve with
                        with_cov=True, .cov
    MapCovariance       the joint covariance of the mapped tags (asl_mapcov_batch): what carries the uncertainty of a
                        map into the covariance of a pose localised against it, which a per-tag std cannot (the tags of a
                        map share their frames, so their errors are correlated)
    MAP_RESULT_DTYPE    asl_map_result
"""
import numpy as np

from ._lib import MAP_RESULT_DTYPE
from .localize import TagMap

STATUS_OK, STATUS_NOTHING, STATUS_NOT_PD, STATUS_NON_FINITE = 0, 1, 2, 3
FRAME_USED, FRAME_FEW_SLOTS, FRAME_DROPPED, FRAME_SOLVE_FAILED, FRAME_NOT_CONNECTED = 0, 1, 3, 4, 5

__all__ = ["MapResult", "MapCovariance", "MAP_RESULT_DTYPE", "STATUS_OK", "STATUS_NOTHING", "STATUS_NOT_PD", "STATUS_NON_FINITE",
           "FRAME_USED", "FRAME_FEW_SLOTS", "FRAME_DROPPED", "FRAME_SOLVE_FAILED", "FRAME_NOT_CONNECTED"]


class MapCovariance:
    """The joint covariance of a map's tags: ids (ascending; neither the world tag, which is the gauge and exact, nor an
    unmapped id) and matrix (6 n, 6 n), block k belonging to ids[k].  Six parameters per tag: (omega, v) of a left update
    of world<-tag in the world frame, MapResult.tag_std's convention, whose squares are the diagonal."""

    def __init__(self, ids, matrix):
        self.ids = [int(i) for i in ids]
        self.matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        if self.ids != sorted(set(self.ids)) or self.matrix.shape != (6 * len(self.ids), 6 * len(self.ids)):
            raise ValueError("ids must be ascending and matrix (6 n, 6 n)")
        self._slot = {i: k for k, i in enumerate(self.ids)}

    @classmethod
    def from_slots(cls, cov_slot, matrix):
        """from the two outputs of asl_mapcov_*: cov_slot (n_ids,) int32 and the matrix (its leading region is read)"""
        cov_slot = np.asarray(cov_slot)
        ids = [int(i) for i in np.flatnonzero(cov_slot >= 0)]
        if [int(cov_slot[i]) for i in ids] != list(range(len(ids))):
            raise ValueError("cov_slot does not number its blocks in ascending id")
        n = 6 * len(ids)
        return cls(ids, np.asarray(matrix)[:n, :n])

    def block(self, i, j):
        """(6, 6) covariance between tags i and j"""
        a, b = 6 * self._slot[int(i)], 6 * self._slot[int(j)]
        return self.matrix[a:a + 6, b:b + 6].copy()

    def marginal(self, i):
        """(6, 6) covariance of tag i alone"""
        return self.block(i, i)

    def std(self, i):
        """(6,) std of tag i: MapResult.tag_std's entry"""
        return np.sqrt(np.diag(self.marginal(i)))

    def cov_slot(self, n_ids):
        """(n_ids,) int32: the block of every id, -1 without one (ids at or past n_ids are left out)"""
        slot = np.full(int(n_ids), -1, dtype=np.int32)
        for i, k in self._slot.items():
            if i < n_ids:
                slot[i] = k
        return slot

    def as_args(self, n_ids):
        """(cov_slot (n_ids,) int32, matrix, ld): d_cov_slot, d_map_cov and its leading dimension as the ABI takes them
        (a matrix without a block is one row of zeros that no slot refers to)"""
        m = self.matrix if len(self.ids) else np.zeros((6, 6))
        return self.cov_slot(n_ids), m, m.shape[1]

    def as_device_args(self, n_ids, device="cuda:0"):
        """as_args as torch tensors on device: (cov_slot, matrix, ld)"""
        import torch
        slot, m, ld = self.as_args(n_ids)
        return torch.from_numpy(slot).to(device), torch.from_numpy(m).to(device), ld

    def save_npz(self, path):
        np.savez(path, ids=np.array(self.ids, dtype=np.int64), matrix=self.matrix)

    @classmethod
    def load_npz(cls, path):
        with np.load(path) as z:
            return cls(z["ids"], z["matrix"])

    def __repr__(self):
        return "MapCovariance(tags=%d)" % len(self.ids)


class MapResult:
    """One map solve: result (MAP_RESULT_DTYPE record), map (n_ids,) MAP_TAG_DTYPE, std (n_ids, 6) or None, poses
    (n_frames,) CAM_POSE_DTYPE; slot_weight (n_frames, max_tags) doubles or None (not computed) with slot_ids, the
    (n_frames, max_tags) ids of the observation block the weights belong to.  From a rig (Rig.build_map) the poses are the
    rig's (world<-rig) and slot_weight / slot_ids are (n_cams, n_frames, max_tags).  cov: a MapCovariance, or None (not
    asked for: build_map(..., with_cov=True))."""

    def __init__(self, result, map_records, tag_std, poses, slot_weight=None, slot_ids=None, cov=None):
        self.result = np.asarray(result, dtype=MAP_RESULT_DTYPE).reshape(())
        self.records = map_records
        self.std = tag_std
        self.poses = poses
        self.slot_weight = slot_weight
        self.slot_ids = slot_ids
        self.cov = cov

    @classmethod
    def from_call(cls, out, slot_ids=None, with_cov=False):
        """from what Detector.build_map / build_map_rig return: the four records, then the slot weights if they were asked
        for, then (with_cov) the (cov_slot, matrix) pair"""
        out = tuple(out)
        cov = MapCovariance.from_slots(*out[-1]) if with_cov else None
        return cls(*(out[:-1] if with_cov else out), slot_ids=slot_ids, cov=cov)

    @property
    def status(self):
        return int(self.result["status"])

    @property
    def ok(self):
        return self.status == STATUS_OK

    @property
    def world_id(self):
        return int(self.result["world_id"])

    @property
    def rms_px(self):
        return float(self.result["rms_px"])

    @property
    def n_soft(self):
        """observations in the solve that the robust loss down-weighted (0 from a plain solve)"""
        return int(self.result["n_soft"])

    def soft_slots(self):
        """[(frame, slot, id, weight)] of every slot with a weight in (0, 1): the observations the robust loss
        down-weighted, in (frame, slot) order; id is -1 without slot_ids.  A rig's solve (Rig.build_map) has a weight
        block (n_cams, n_frames, max_tags) and gives [(camera, frame, slot, id, weight)] in (camera, frame, slot) order."""
        if self.slot_weight is None:
            raise ValueError("the slot weights were not computed (build_map(..., huber_px=k))")
        w = np.asarray(self.slot_weight)
        return [tuple(int(i) for i in k) + (int(self.slot_ids[tuple(k)]) if self.slot_ids is not None else -1, float(w[tuple(k)]))
                for k in np.argwhere((w > 0) & (w < 1))]

    @property
    def tag_map(self):
        """TagMap of the mapped tags (world<-tag, the world tag at the identity)"""
        return TagMap.from_records(self.records)

    @property
    def tag_std(self):
        """{id: (6,) std of (omega, v) of a left update in the world frame}; zeros for the world tag"""
        if self.std is None:
            return {}
        return {int(i): np.array(self.std[i]) for i in np.flatnonzero(self.records["valid"])}

    @property
    def camera_poses(self):
        """(n_frames, 4, 4) world<-camera (a rig's solve: world<-rig); the identity where frame_status is not 0 or 4"""
        return np.array(self.poses["T"])

    @property
    def frame_status(self):
        return np.array(self.poses["status"])

    def __repr__(self):
        return "MapResult(status=%d, world_id=%d, tags=%d, frames=%d, rms_px=%.4g)" % (
            self.status, self.world_id, int(self.result["n_tags"]), int(self.result["n_frames_used"]), self.rms_px)
