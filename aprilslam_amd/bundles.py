"""Tag bundles: several rigid objects that each carry a few tags, every one posed in every frame by one call
(asl_localize_bundles_batch / asl_localize_bundles_frames_device and the rig forms, k_localize.inc; asl_bundle_relative_*,
k_bundle.inc).

A bundle is the tag layout of one object in the object's own frame, a localize.TagMap with bundle<-tag poses.  The solve
of frame f against bundle b is the localisation of that frame with the bundle as the world, so the pose it returns is
bundle<-camera (bundle<-rig for a rig); a frame that sees no tag of the bundle has status 1 there.

    BundleSet       the bundles of a call, in order: table(n_ids) -> (n_bundles, n_ids) MAP_TAG_DTYPE, save / load,
                    from_map() (bundle calibration: cut one built map into bundles)
    BundleResult    what the localize_bundles calls return: T[f, b], status, cov, relative(ref), pose_std()
    BUNDLE_REL_DTYPE  one asl_bundle_rel per (frame, bundle): T = ref<-bundle, cov 6x6 in the convention of POSE_COV_DTYPE, status

The covariances take the bundles' layouts as exact, and the covariance of a relative pose takes the two poses as
independent: their solves share no corner, because no tag id is valid in two bundles (BundleSet refuses that).
"""
import numpy as np

from ._lib import BUNDLE_REL_DTYPE, CAM_POSE_DTYPE, MAP_TAG_DTYPE, POSE_COV_DTYPE
from .localize import TagMap, pose_std

MAX_BUNDLES = 1024

REL_OK, REL_NO_POSE, REL_NO_COV = 0, 1, 2

__all__ = ["BundleSet", "BundleResult", "BUNDLE_REL_DTYPE", "MAX_BUNDLES", "REL_OK", "REL_NO_POSE", "REL_NO_COV"]


class BundleSet:
    """The bundles of a call, each a localize.TagMap of bundle<-tag poses (with the tags' own sizes where set), and their
    names (default "0", "1", ...).  An id that is valid in two bundles is a ValueError: the two solves would share its
    corners, and the covariance of their relative pose takes them as independent."""

    def __init__(self, maps, names=None):
        self.maps = list(maps)
        if not 1 <= len(self.maps) <= MAX_BUNDLES or not all(isinstance(m, TagMap) for m in self.maps):
            raise ValueError("a BundleSet has 1 to %d TagMap" % MAX_BUNDLES)
        self.names = [str(k) for k in range(len(self.maps))] if names is None else [str(n) for n in names]
        if len(self.names) != len(self.maps) or len(set(self.names)) != len(self.names):
            raise ValueError("one distinct name per bundle")
        owner = {}
        for b, m in enumerate(self.maps):
            for i in m.ids():
                if i in owner:
                    raise ValueError("tag id %d is valid in bundles %s and %s" % (i, self.names[owner[i]], self.names[b]))
                owner[i] = b
        self._owner = owner

    def __len__(self):
        return len(self.maps)

    def __getitem__(self, b):
        return self.maps[self.index(b)]

    def index(self, b):
        """the position of a bundle given by position or by name"""
        if isinstance(b, str):
            return self.names.index(b)
        b = int(b)
        if not 0 <= b < len(self.maps):
            raise IndexError("bundle %d of %d" % (b, len(self.maps)))
        return b

    def bundle_of(self, tag_id):
        """the position of the bundle that carries tag_id, None if none does"""
        return self._owner.get(int(tag_id))

    @property
    def n_ids(self):
        """length of the id-indexed tables: the largest id of any bundle + 1"""
        return max(m.n_ids for m in self.maps)

    def table(self, n_ids=None):
        """(n_bundles, n_ids) MAP_TAG_DTYPE, C-contiguous: row b is bundle b's TagMap.as_records(), valid = 0 for the ids it
        does not carry.  n_ids None: self.n_ids; ids at or above a given n_ids are left out, as the solvers ignore them."""
        n = max(self.n_ids if n_ids is None else int(n_ids), 1)
        t = np.zeros((len(self.maps), n), dtype=MAP_TAG_DTYPE)
        for b, m in enumerate(self.maps):
            rec = m.as_records()[:n]
            t[b, :len(rec)] = rec
        return t

    @classmethod
    def from_map(cls, tag_map, groups, origins=None, names=None):
        """Bundle calibration: cut one map (a TagMap or MAP_TAG_DTYPE records, e.g. build_map of a recording with all objects
        at rest) into one bundle per group of ids, each re-expressed in its own frame:
        bundle<-tag = inv(world<-origin_tag) world<-tag.  origins: the origin tag of each group (None: its lowest id), which
        sits at the identity of its bundle.  Sizes are carried over.  Host NumPy only."""
        tm = tag_map if isinstance(tag_map, TagMap) else TagMap.from_records(tag_map)
        groups = [sorted(int(i) for i in g) for g in groups]
        if origins is None:
            origins = [None] * len(groups)
        if len(origins) != len(groups):
            raise ValueError("one origin per group")
        maps = []
        for g, origin in zip(groups, origins):
            if not g:
                raise ValueError("a bundle has at least one tag")
            origin = g[0] if origin is None else int(origin)
            missing = [i for i in g if i not in tm]
            if origin not in g or missing:
                raise ValueError("origin %d must be in its group %s, and every id of the group in the map (missing: %s)" % (origin, g, missing))
            inv = np.linalg.inv(tm[origin])
            m = TagMap({i: inv @ tm[i] for i in g}, {i: tm.size(i) for i in g})
            m[origin] = np.eye(4)
            maps.append(m)
        return cls(maps, names)

    def save(self, path):
        """Write the set to an .npz file: names (n_bundles,), and per tag its bundle (n,), id (n,), T (n, 4, 4) bundle<-tag and
        size (n,) float32 (0: none), in bundle then id order."""
        rows = [(b, i, m[i], m.size(i)) for b, m in enumerate(self.maps) for i in m.ids()]
        np.savez(path, names=np.array(self.names), bundle=np.array([r[0] for r in rows], dtype=np.int64),
                 ids=np.array([r[1] for r in rows], dtype=np.int64), T=np.array([r[2] for r in rows], dtype=np.float64).reshape(-1, 4, 4),
                 sizes=np.array([r[3] for r in rows], dtype=np.float32))

    @classmethod
    def load(cls, path):
        """The set BundleSet.save wrote."""
        with np.load(path) as z:
            names, bundle, ids, T, sizes = z["names"], z["bundle"], z["ids"], z["T"], z["sizes"]
            n = len(ids)
            if names.ndim != 1 or bundle.shape != (n,) or T.shape != (n, 4, 4) or sizes.shape != (n,) or (n and not 0 <= bundle.min() <= bundle.max() < len(names)):
                raise ValueError("%s is not a saved BundleSet (names (n_bundles,), bundle, ids, sizes (n,), T (n, 4, 4))" % path)
            maps = [TagMap({int(ids[k]): T[k] for k in np.flatnonzero(bundle == b)}, {int(ids[k]): sizes[k] for k in np.flatnonzero(bundle == b)})
                    for b in range(len(names))]
            return cls(maps, [str(s) for s in names])


class BundleResult:
    """What the localize_bundles calls return.  poses: (n_frames, n_bundles) CAM_POSE_DTYPE with T[f, b] = bundle_b<-camera
    (bundle_b<-rig); cov: their (n_frames, n_bundles) POSE_COV_DTYPE, or None without with_cov; det: the _lib.Detector
    that relative() runs on."""

    def __init__(self, poses, cov=None, bundles=None, det=None):
        self.poses = np.asarray(poses, dtype=CAM_POSE_DTYPE)
        self.cov_records = None if cov is None else np.asarray(cov, dtype=POSE_COV_DTYPE)
        self.bundles, self._det = bundles, det

    @property
    def T(self):
        """(n_frames, n_bundles, 4, 4): bundle<-camera; the identity where status is not 0"""
        return self.poses["T"]

    @property
    def status(self):
        """(n_frames, n_bundles): 0 posed, 1 no tag of the bundle in view, 2 no tag of it with a successful PnP"""
        return self.poses["status"]

    @property
    def cov(self):
        """(n_frames, n_bundles, 6, 6) in the order (rx ry rz | px py pz), zeros where cov_status is not 0; None without with_cov"""
        return None if self.cov_records is None else self.cov_records["cov"]

    @property
    def cov_status(self):
        return None if self.cov_records is None else self.cov_records["status"]

    def pose_std(self):
        """(rotation std in rad, translation std), each (n_frames, n_bundles, 3): localize.pose_std of cov"""
        if self.cov_records is None:
            raise ValueError("no covariance: localise with with_cov=True")
        return pose_std(self.cov)

    def relative(self, ref):
        """(n_frames, n_bundles) BUNDLE_REL_DTYPE: T = ref<-bundle with its covariance for every frame and bundle, ref a
        position or, with a BundleSet, a name (Detector.bundle_relative, asl_bundle_relative_batch).  status 1 where the
        bundle or the reference has no pose in the frame, 2 (T valid, cov zeros) where a covariance is missing.  With a
        mapped world as one of the bundles, relative(that one) is the pose of every object in the world."""
        if self._det is None:
            raise ValueError("this result has no detector to run on")
        r = self.bundles.index(ref) if self.bundles is not None else int(ref)
        return self._det.bundle_relative(self.poses, self.cov_records, r)
