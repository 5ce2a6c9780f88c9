"""Tag-map reconstruction from a batch of frames (asl_map_batch / asl_map_frames_device).

Frames that see an unknown set of tags give the tags' world<-tag poses (the world tag at the identity), every frame's
camera pose and a per-tag standard deviation; the map is the asl_map_tag block localisation reads (localize.TagMap).

    MapResult           the records of one solve, with .tag_map, .tag_std, .camera_poses, .frame_status and, from a solve
                        with a robust loss (huber_px), .n_soft, .slot_weight and .soft_slots()
    MAP_RESULT_DTYPE    asl_map_result
"""
import numpy as np

from ._lib import MAP_RESULT_DTYPE
from .localize import TagMap

STATUS_OK, STATUS_NOTHING, STATUS_NOT_PD, STATUS_NON_FINITE = 0, 1, 2, 3
FRAME_USED, FRAME_FEW_SLOTS, FRAME_DROPPED, FRAME_SOLVE_FAILED, FRAME_NOT_CONNECTED = 0, 1, 3, 4, 5

__all__ = ["MapResult", "MAP_RESULT_DTYPE", "STATUS_OK", "STATUS_NOTHING", "STATUS_NOT_PD", "STATUS_NON_FINITE",
           "FRAME_USED", "FRAME_FEW_SLOTS", "FRAME_DROPPED", "FRAME_SOLVE_FAILED", "FRAME_NOT_CONNECTED"]


class MapResult:
    """One map solve: result (MAP_RESULT_DTYPE record), map (n_ids,) MAP_TAG_DTYPE, std (n_ids, 6) or None, poses
    (n_frames,) CAM_POSE_DTYPE; slot_weight (n_frames, max_tags) doubles or None (not computed) with slot_ids, the
    (n_frames, max_tags) ids of the observation block the weights belong to.  From a rig (Rig.build_map) the poses are the
    rig's (world<-rig) and slot_weight / slot_ids are (n_cams, n_frames, max_tags)."""

    def __init__(self, result, map_records, tag_std, poses, slot_weight=None, slot_ids=None):
        self.result = np.asarray(result, dtype=MAP_RESULT_DTYPE).reshape(())
        self.records = map_records
        self.std = tag_std
        self.poses = poses
        self.slot_weight = slot_weight
        self.slot_ids = slot_ids

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
