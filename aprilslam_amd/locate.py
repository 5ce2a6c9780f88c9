"""Extending a tag map: the world<-tag pose of tags the map does not have, from frames whose camera poses are known
(asl_locate_tags_batch / asl_locate_tags_frames_device, k_locate.inc).

Localisation takes the map as exact and solves a frame's camera; this is its dual: each unmapped tag is solved on its own
from all its views with the cameras held fixed.  The known tags are never moved, so the gauge and every pose the rest of a
system relies on stay as they are.  The result is not the joint optimum of cameras and tags: the frame poses are taken as
exact and their uncertainty is not propagated.

    LocateResult    the records of one call, with .tag_map, .located_ids, .status and .tag_std()
    extend_map      localise a block of frames against the map, then locate every tag the map does not have
    wanted_records  the record block of such a call: the map grown to every id seen, the known sizes written in
                    (rig.Rig.extend_map, the rig form over asl_locate_tags_rig_*, calls it too)
    TAG_FIT_DTYPE   one asl_tag_fit per id: rms_px, rms_seed_px, n_views, n_rejected, status, seed_frame, seed_mirrored
"""
import numpy as np

from ._lib import MAP_TAG_DTYPE, TAG_FIT_DTYPE, _map_records, _obs_records
from .localize import TagMap, pose_std

STATUS_LOCATED, STATUS_NOT_WANTED, STATUS_FEW_VIEWS, STATUS_NO_PNP = 0, 1, 2, 3

__all__ = ["LocateResult", "extend_map", "wanted_records", "TAG_FIT_DTYPE", "STATUS_LOCATED", "STATUS_NOT_WANTED", "STATUS_FEW_VIEWS", "STATUS_NO_PNP"]


class LocateResult:
    """One locate call: records (n_ids,) MAP_TAG_DTYPE, the extended map as the solvers read it; fit (n_ids,) TAG_FIT_DTYPE;
    cov_records (n_ids,) POSE_COV_DTYPE or None (not computed)."""

    def __init__(self, records, fit, cov_records=None):
        self.records = records
        self.fit = fit
        self.cov_records = cov_records

    @property
    def tag_map(self):
        """TagMap of the extended map: the entries that were valid and the located ones, with their sizes"""
        return TagMap.from_records(self.records)

    @property
    def located_ids(self):
        return [int(i) for i in np.flatnonzero(self.fit["status"] == STATUS_LOCATED)]

    @property
    def status(self):
        """per id: 0 located, 1 not wanted, 2 fewer than min_views views, 3 no view with a PnP"""
        return np.array(self.fit["status"])

    def tag_std(self):
        """{id: (rotation std in rad (3), translation std (3))} of every located tag whose covariance is good
        (localize.pose_std of world<-tag: rotation about the world axes, translation of the tag's position)"""
        if self.cov_records is None:
            raise ValueError("the covariance was not computed (sigma_px=...)")
        return {i: pose_std(self.cov_records["cov"][i]) for i in self.located_ids if self.cov_records["status"][i] == 0}

    def __repr__(self):
        return "LocateResult(located=%d, wanted=%d)" % (len(self.located_ids), int((self.fit["status"] != STATUS_NOT_WANTED).sum()))


def extend_map(det, obs, tag_map, K, dist, tag_size, tag_sizes=None, max_view_rms_px=0.0, min_views=2, sigma_px=None, max_tag_rms_px=0.0):
    """Host records obs (n_frames, max_tags) OBS_DTYPE and a map (a TagMap, or (n_ids,) MAP_TAG_DTYPE) that has some of the
    tags they see -> (LocateResult, (n_frames,) CAM_POSE_DTYPE): the frames are localised against the map
    (_lib.Detector.localize, gate max_tag_rms_px), then every id the map does not have is located from the frames that got
    a pose (_lib.Detector.locate_tags, gate max_view_rms_px).  The record block grows to cover every id seen.  tag_sizes
    ({id: size}): the known side of unmapped tags that is not tag_size; it is written into their entries, which the located
    tags keep.  The entries the map had come back byte for byte."""
    o = _obs_records(obs)
    rec = wanted_records(o, tag_map, tag_sizes)
    poses = det.localize(o, rec, K, dist, tag_size, max_tag_rms_px=max_tag_rms_px)
    out, fit, cov = det.locate_tags(o, poses, rec, K, dist, tag_size, max_view_rms_px=max_view_rms_px, min_views=min_views, sigma_px=sigma_px)
    return LocateResult(out, fit, cov), poses


def wanted_records(o, tag_map, tag_sizes=None):
    """The record block extend_map (and rig.Rig.extend_map) hands to the solvers: a copy of tag_map's records, grown to
    cover every id the asl_obs records o (any shape) see, with tag_sizes ({id: size}) written into the entries that have
    no pose.  The entries the map had keep their bytes."""
    rec = _map_records(tag_map)
    seen = o["id"][(o["flags"] & 1) != 0]
    n_ids = max(len(rec), int(seen.max()) + 1 if seen.size else 1, 1)
    if n_ids > len(rec):
        grown = np.zeros(n_ids, dtype=MAP_TAG_DTYPE)
        grown[:len(rec)] = rec
        rec = grown
    else:
        rec = rec.copy()
    for i, size in (tag_sizes or {}).items():
        i, size = int(i), float(np.float32(size))
        if not (np.isfinite(size) and size >= 0):
            raise ValueError("a tag size is finite and non-negative (0: the call's tag_size)")
        if 0 <= i < n_ids and not rec["valid"][i]:
            rec["size"][i] = size   # an id without a pose: TagMap.set_size has no place for it
    return rec
