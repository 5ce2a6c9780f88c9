"""Camera localisation against a known map of tag poses (asl_localize_batch / asl_localize_frames_device).

A frame that sees n mapped tags gives 8n pixel residuals for the 6 unknowns of its camera pose; the joint solve
(k_localize.inc: best single-view seed -> Levenberg-Marquardt over every tag's corners) is far better conditioned than
any one tag's planar PnP.  The map may come from SLAM.optimize() (SLAM.tag_map()), from a survey or from a synthetic
scene (TagMap.from_scene).

    TagMap          ids -> world<-tag 4x4 and, optionally, the tag's own side length, as the asl_map_tag records the
                    library reads (indexed by id)
    CAM_POSE_DTYPE  one asl_cam_pose per frame: world<-camera T, rms_px, rms_seed_px, n_tags, n_rejected, status, seed_slot
    POSE_COV_DTYPE  one asl_pose_cov per pose: cov 6x6 (rx ry rz | px py pz), sigma_px, dof, status; pose_std reads it
    BUNDLE_REL_DTYPE  one asl_bundle_rel per (frame, bundle): T = ref<-bundle, cov 6x6, status (bundles.py: several maps at once)
"""
import numpy as np

from ._lib import BUNDLE_REL_DTYPE, CAM_POSE_DTYPE, MAP_TAG_DTYPE, POSE_COV_DTYPE

STATUS_OK, STATUS_NO_MAPPED_TAG, STATUS_NO_PNP = 0, 1, 2

COV_OK, COV_NO_POSE, COV_NOT_POSITIVE_DEFINITE = 0, 1, 2

__all__ = ["TagMap", "CAM_POSE_DTYPE", "MAP_TAG_DTYPE", "POSE_COV_DTYPE", "BUNDLE_REL_DTYPE", "STATUS_OK", "STATUS_NO_MAPPED_TAG", "STATUS_NO_PNP",
           "COV_OK", "COV_NO_POSE", "COV_NOT_POSITIVE_DEFINITE", "pose_std"]


def pose_std(cov):
    """(rotation std in rad (3), translation std (3)) of a 6x6 pose covariance in the order (rx ry rz | px py pz), or of a
    stack of them (..., 6, 6): the roots of the diagonal.  Rotation about the axes of the pose's target frame, translation
    of its translation column (include/aprilslam.h: asl_pose_cov)."""
    d = np.sqrt(np.diagonal(np.asarray(cov, dtype=np.float64), axis1=-2, axis2=-1))
    return d[..., :3], d[..., 3:]


class TagMap:
    """World<-tag poses by tag id.  The tag frame is the one the per-tag PnP reports (camera<-tag): corners at (+-h, +-h, 0)
    in the order lb, rb, rt, lt.  h is half the call's tag_size, or half the tag's own size where one is set (set_size):
    every solver that takes a map honours it."""

    def __init__(self, poses=None, sizes=None):
        self.poses = {}
        self.sizes = {}
        for tag_id, T in (poses or {}).items():
            self[tag_id] = T
        for tag_id, size in (sizes or {}).items():
            self.set_size(tag_id, size)

    def __setitem__(self, tag_id, T):
        tag_id = int(tag_id)
        if tag_id < 0:
            raise ValueError("tag ids are non-negative")
        T = np.array(T, dtype=np.float64)
        if T.shape == (3, 4):
            T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
        if T.shape != (4, 4) or not np.all(np.isfinite(T)):
            raise ValueError("a map pose is a finite 4x4 (or 3x4) world<-tag transform")
        self.poses[tag_id] = T

    def __getitem__(self, tag_id):
        return self.poses[int(tag_id)]

    def set_size(self, tag_id, size):
        """The side of tag tag_id, in the units and with the meaning of the solvers' tag_size (between the corner points
        the detector reports), kept as float32 like the record's field.  0 clears it: the tag then has the call's tag_size."""
        tag_id = int(tag_id)
        if tag_id not in self.poses:
            raise KeyError("tag %d has no pose in this map" % tag_id)
        size = float(np.float32(size))
        if not (np.isfinite(size) and size >= 0):
            raise ValueError("a tag size is finite and non-negative (0: the call's tag_size)")
        if size == 0:
            self.sizes.pop(tag_id, None)
        else:
            self.sizes[tag_id] = size

    def size(self, tag_id):
        """The tag's own side, 0.0 if none is set (the tag has the call's tag_size)."""
        return self.sizes.get(int(tag_id), 0.0)

    def tag_pose(self, tag_id, T_cam_tag, tag_size):
        """camera<-tag (4x4) of tag tag_id from the pose T_cam_tag that the per-tag PnP gave at tag_size (get_pose, or a
        record's T).  For a tag with a size of its own the rotation holds and the translation is multiplied by
        k = float32(size / 2) / float32(tag_size / 2): object and translation scaled together leave every ray where it
        is, under any lens.  A tag without a size comes back unchanged."""
        T = np.array(T_cam_tag, dtype=np.float64)
        if T.shape == (3, 4):
            T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
        size = self.size(tag_id)
        if size > 0:
            T[:3, 3] *= float(np.float32(size) * np.float32(0.5)) / float(np.float32(tag_size / 2))
        return T

    def __contains__(self, tag_id):
        return int(tag_id) in self.poses

    def __len__(self):
        return len(self.poses)

    def ids(self):
        return sorted(self.poses)

    @property
    def n_ids(self):
        """length of the id-indexed record array: max id + 1"""
        return max(self.poses) + 1 if self.poses else 0

    @classmethod
    def from_dict(cls, poses):
        """{id: world<-tag 4x4 (or 3x4)}"""
        return cls(poses)

    @classmethod
    def from_scene(cls, tags):
        """tags of synth.random_scene / default_scene ({"id", "position", "rotation"}): the scene's world frame with
        synth.tag_model_matrix as the tag frame -- the frame in which synth's ground truth camera<-tag poses are given."""
        from .synth import tag_model_matrix
        return cls({int(t["id"]): tag_model_matrix(t["position"], t["rotation"]) for t in tags})

    @classmethod
    def grid(cls, rows, cols, tag_size, spacing, first_id=0):
        """A planar board of rows x cols tags in the board's z = 0 plane, tag axes along the board's: the tag of row r and
        column c has id first_id + r * cols + c and its centre at (c * spacing, r * spacing, 0).  spacing is the distance
        between neighbouring tag centres; tag_size (the side the PnP uses) must fit into it."""
        rows, cols, first_id = int(rows), int(cols), int(first_id)
        if rows < 1 or cols < 1 or first_id < 0:
            raise ValueError("a grid has rows, cols >= 1 and first_id >= 0")
        if not (tag_size > 0 and spacing >= tag_size):
            raise ValueError("tag_size must be positive and spacing >= tag_size")
        poses = {}
        for r in range(rows):
            for c in range(cols):
                T = np.eye(4)
                T[0, 3], T[1, 3] = c * float(spacing), r * float(spacing)
                poses[first_id + r * cols + c] = T
        return cls(poses)

    def save(self, path):
        """Write the map to an .npz file: ids (n,), T (n, 4, 4) world<-tag and sizes (n,) float32 (0: none), in ascending
        id order."""
        ids = self.ids()
        T = np.array([self.poses[i] for i in ids], dtype=np.float64).reshape(-1, 4, 4)
        sizes = np.array([self.size(i) for i in ids], dtype=np.float32)
        np.savez(path, ids=np.array(ids, dtype=np.int64), T=T, sizes=sizes)

    @classmethod
    def load(cls, path):
        """The map TagMap.save wrote; a file without sizes (written before tags had them) gives sizes of 0."""
        with np.load(path) as z:
            ids, T = z["ids"], z["T"]
            if ids.ndim != 1 or T.shape != (len(ids), 4, 4):
                raise ValueError("%s is not a saved TagMap (ids (n,), T (n, 4, 4))" % path)
            sizes = z["sizes"] if "sizes" in z.files else np.zeros(len(ids), dtype=np.float32)
            if sizes.shape != (len(ids),):
                raise ValueError("%s: sizes must be (n,) like ids" % path)
            return cls({int(i): T[k] for k, i in enumerate(ids)}, {int(i): sizes[k] for k, i in enumerate(ids)})

    @classmethod
    def from_records(cls, rec):
        """The valid entries of an (n_ids,) MAP_TAG_DTYPE block (e.g. asl_map_frames_device's output), with their sizes.
        An entry with a negative or non-finite size counts as not valid, as in the solvers."""
        rec = np.asarray(rec, dtype=MAP_TAG_DTYPE).ravel()
        ok = (rec["valid"] != 0) & np.isfinite(rec["size"]) & (rec["size"] >= 0)
        return cls({int(i): rec["T"][i].reshape(3, 4) for i in np.flatnonzero(ok)}, {int(i): rec["size"][i] for i in np.flatnonzero(ok)})

    def as_records(self):
        """(n_ids,) MAP_TAG_DTYPE, indexed by id; ids without a pose have valid = 0, tags without a size have size = 0"""
        rec = np.zeros(max(self.n_ids, 1), dtype=MAP_TAG_DTYPE)
        for tag_id, T in self.poses.items():
            rec["T"][tag_id] = T[:3].ravel()
            rec["valid"][tag_id] = 1
            rec["size"][tag_id] = self.size(tag_id)
        return rec
