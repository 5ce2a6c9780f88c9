"""Several cameras on one rigid body localised together against a tag map (asl_localize_rig_batch /
asl_localize_rig_frames_device, k_rig.inc).

One pose world<-rig per frame from every camera's corners in one solve: cameras that each see one or two small tags
(each alone badly conditioned in tilt, or without any tag for a few frames) constrain one another through the known
mounting.  A frame index is one instant for all cameras.

    RigCamera       one camera: K, dist (0, 4 or 5 coefficients), T_cam_rig = camera<-rig 4x4 (the mounting)
    Rig             the cameras in block order; as_records() -> RIG_CAMERA_DTYPE (asl_rig_camera), save / load,
                    localize(), localize_bundles(), localize_sequence() / localize_sequences(), build_map() / build_map_sized(),
                    locate_tags() / extend_map(), from_camera_poses(), calibrate_mountings()
    RigCalibrationResult   what calibrate_mountings returns: the refined Rig, the result record, the mountings' covariances
                    and the frames' poses

Consecutive frames of the rig solved together under a random-walk motion prior (asl_smooth_rig_sequences_batch, k_smooth.inc):
Rig.localize_sequence and Rig.localize_sequences return smooth.SmoothResult, its poses the rig's (world<-rig).  A frame in
which no camera sees a mapped tag is carried by its neighbours, a frame whose only tag is one small tag in one camera is
kept out of its mirrored planar minimum by them, and corner noise is averaged over the sequence.
"""
import numpy as np

from ._lib import CAM_POSE_DTYPE, OBS_DTYPE, RIG_CAMERA_DTYPE
from .smooth import SmoothResult

MAX_CAMERAS = 16
MAX_SLOTS = 256          # n_cams * max_tags
ORTHONORMAL_TOL = 1e-6

MAX_CALIBRATED_CAMERAS = 8   # calibrate_mountings

__all__ = ["Rig", "RigCamera", "RigCalibrationResult", "RIG_CAMERA_DTYPE", "MAX_CAMERAS", "MAX_SLOTS", "MAX_CALIBRATED_CAMERAS"]


def _transform(T, what):
    T = np.array(T, dtype=np.float64)
    if T.shape == (3, 4):
        T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError("%s is a finite 4x4 (or 3x4) transform" % what)
    R = T[:3, :3]
    if np.abs(R @ R.T - np.eye(3)).max() > ORTHONORMAL_TOL or not np.linalg.det(R) > 0:
        raise ValueError("the rotation part of %s is not a rotation" % what)
    T[3] = [0.0, 0.0, 0.0, 1.0]
    return T


class RigCamera:
    """One camera of a rig: its pinhole + lens model and its mounting T_cam_rig = camera<-rig."""

    def __init__(self, K, dist=None, T_cam_rig=None):
        self.K = np.array(K, dtype=np.float64)
        if self.K.shape != (3, 3) or not np.all(np.isfinite(self.K)):
            raise ValueError("K must be a finite 3x3 matrix")
        self.dist = np.array([] if dist is None else dist, dtype=np.float64).ravel()
        if len(self.dist) not in (0, 4, 5) or not np.all(np.isfinite(self.dist)):
            raise ValueError("dist must have 0, 4 or 5 finite coefficients")
        self.T_cam_rig = _transform(np.eye(4) if T_cam_rig is None else T_cam_rig, "T_cam_rig")


class Rig:
    """The cameras of a rig, in the order of the observation block's leading axis."""

    def __init__(self, cameras):
        self.cameras = list(cameras)
        if not 1 <= len(self.cameras) <= MAX_CAMERAS or not all(isinstance(c, RigCamera) for c in self.cameras):
            raise ValueError("a rig has 1 to %d RigCamera" % MAX_CAMERAS)

    def __len__(self):
        return len(self.cameras)

    def as_records(self):
        """(n_cams,) RIG_CAMERA_DTYPE: the table the library reads"""
        rec = np.zeros(len(self.cameras), dtype=RIG_CAMERA_DTYPE)
        for k, c in enumerate(self.cameras):
            rec["K"][k] = c.K
            rec["dist"][k][:len(c.dist)] = c.dist
            rec["E"][k] = c.T_cam_rig[:3]
            rec["n_dist"][k] = len(c.dist)
        return rec

    @classmethod
    def from_records(cls, rec):
        rec = np.asarray(rec, dtype=RIG_CAMERA_DTYPE).ravel()
        return cls([RigCamera(r["K"], r["dist"][:r["n_dist"]], r["E"]) for r in rec])

    def save(self, path):
        """Write the rig to an .npz file: K (n, 3, 3), dist (n, 5), n_dist (n,), T_cam_rig (n, 4, 4)."""
        rec = self.as_records()
        np.savez(path, K=rec["K"], dist=rec["dist"], n_dist=rec["n_dist"].astype(np.int64),
                 T_cam_rig=np.array([c.T_cam_rig for c in self.cameras], dtype=np.float64))

    @classmethod
    def load(cls, path):
        """The rig Rig.save wrote."""
        with np.load(path) as z:
            K, dist, nd, T = z["K"], z["dist"], z["n_dist"], z["T_cam_rig"]
            n = len(nd)
            if nd.ndim != 1 or K.shape != (n, 3, 3) or dist.shape != (n, 5) or T.shape != (n, 4, 4):
                raise ValueError("%s is not a saved Rig (K (n, 3, 3), dist (n, 5), n_dist (n,), T_cam_rig (n, 4, 4))" % path)
            return cls([RigCamera(K[k], dist[k][:int(nd[k])], T[k]) for k in range(n)])

    def localize(self, det, obs, tag_map, tag_size, max_tag_rms_px=0.0, with_cov=False, sigma_px=0.0, map_cov=None):
        """obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, against tag_map (a localize.TagMap or MAP_TAG_DTYPE
        records) on det (a _lib.Detector) -> (n_frames,) CAM_POSE_DTYPE with T = world<-rig; with_cov: (poses, (n_frames,)
        POSE_COV_DTYPE), scaled by sigma_px or, for 0, by the solve's own estimate.  tag_size is the size of the map entries
        that have none of their own (TagMap.set_size), here and in localize_sequence / localize_sequences.  map_cov (with
        with_cov; a mapping.MapCovariance, e.g. build_map(with_cov=True).cov): the uncertainty of the map's tags is carried
        into the covariances (asl_localize_rig_mapcov_batch)."""
        if map_cov is not None and not with_cov:
            raise ValueError("map_cov needs with_cov=True")
        o = np.asarray(obs)
        if o.dtype != OBS_DTYPE or o.ndim != 3 or o.shape[0] != len(self.cameras):
            raise ValueError("obs must be (%d, n_frames, max_tags) asl_obs records" % len(self.cameras))
        if o.shape[0] * o.shape[2] > MAX_SLOTS:
            raise ValueError("n_cams * max_tags must be <= %d" % MAX_SLOTS)
        return det.localize_rig(o, tag_map, self.as_records(), tag_size, max_tag_rms_px, float(sigma_px) if with_cov else None, map_cov=map_cov)

    def localize_bundles(self, det, obs, bundles, tag_size, max_tag_rms_px=0.0, with_cov=False, sigma_px=0.0):
        """Every bundle of a bundles.BundleSet posed in every frame by one call (Detector.localize_bundles_rig,
        asl_localize_bundles_rig_batch): obs as in localize -> bundles.BundleResult with T[f, b] = bundle_b<-rig, entry [f, b]
        what localize gives for frame f with bundle b as the map; with_cov: with the covariances, which relative() carries
        into those of the relative poses."""
        from .bundles import BundleResult
        got = det.localize_bundles_rig(self._block(obs), bundles, self.as_records(), tag_size, max_tag_rms_px, float(sigma_px) if with_cov else None)
        return BundleResult(got[0], got[1], bundles, det) if with_cov else BundleResult(got, None, bundles, det)

    def build_map(self, det, obs, n_ids, tag_size, world_id=-1, max_iters=30, with_std=True, huber_px=0.0):
        """The tag map from the rig's own frames (Detector.build_map_rig, asl_map_rig_batch): obs (n_cams, n_frames, max_tags)
        OBS_DTYPE, camera-major, of tags with ids below n_ids at unknown poses -> mapping.MapResult: the world<-tag map (the
        world tag world_id, default the lowest id seen, at the identity), the per-tag std and one pose per frame,
        camera_poses = world<-rig.  Every camera's views enter one solve through the mountings, which are taken as exact, so
        tags that no single camera sees together share one map.  huber_px > 0: a Huber loss of that many pixels on every
        corner residual; the result's soft_slots() are then (camera, frame, slot, id, weight).  Tags of different known
        sizes: build_map_sized.  With the joint covariance of the mapped tags: build_map_cov."""
        return self.build_map_sized(det, obs, n_ids, tag_size, None, world_id=world_id, max_iters=max_iters, with_std=with_std, huber_px=huber_px)

    def build_map_cov(self, det, obs, n_ids, tag_size, tag_sizes=None, world_id=-1, max_iters=30, huber_px=0.0):
        """build_map / build_map_sized with the joint covariance of the mapped tags as result.cov, a mapping.MapCovariance
        (asl_mapcov_rig_batch): what localize(with_cov=True, map_cov=result.cov) carries into the covariance of a rig pose."""
        return self.build_map_sized(det, obs, n_ids, tag_size, tag_sizes, world_id=world_id, max_iters=max_iters, huber_px=huber_px, with_cov=True)

    def build_map_sized(self, det, obs, n_ids, tag_size, tag_sizes, world_id=-1, max_iters=30, with_std=True, huber_px=0.0, with_cov=False):
        """build_map for tags of different known sizes (asl_map_rig_sized_batch): tag_sizes is a {id: size} dict or an array of
        n_ids sizes, 0 or an id not named standing for tag_size (None: build_map itself).  Every tag is solved at its own
        size and the result's tag_map carries the sizes, so that localize() and localize_sequences() against it honour them.
        with_cov: build_map_cov."""
        from .mapping import MapResult
        o = self._block(obs)
        out = det.build_map_rig(o, n_ids, self.as_records(), tag_size, world_id=world_id, max_iters=max_iters, with_std=with_std,
                                huber_px=huber_px, with_slot_weight=bool(huber_px), tag_sizes=tag_sizes, with_cov=with_cov)
        return MapResult.from_call(out, slot_ids=o["id"] if huber_px else None, with_cov=with_cov)

    def locate_tags(self, det, obs, poses, tag_map, tag_size, max_view_rms_px=0.0, min_views=2, sigma_px=None):
        """The tags the map does not have, located from the rig's posed frames (Detector.locate_tags_rig,
        asl_locate_tags_rig_batch): obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, poses (n_frames,)
        CAM_POSE_DTYPE with T = world<-rig (localize(), localize_sequence() or build_map()'s camera_poses) ->
        locate.LocateResult.  Every camera's view of a tag is a view of its own through that camera's mounting, so a tag
        that only a camera without a mapped tag in view sees is located too, and one two cameras see at the same instant
        is solved from both.  The mountings and the poses are taken as exact."""
        from .locate import LocateResult
        return LocateResult(*det.locate_tags_rig(self._block(obs), poses, tag_map, self.as_records(), tag_size, max_view_rms_px=max_view_rms_px,
                                                 min_views=min_views, sigma_px=sigma_px))

    def extend_map(self, det, obs, tag_map, tag_size, tag_sizes=None, max_view_rms_px=0.0, min_views=2, sigma_px=None, max_tag_rms_px=0.0):
        """locate.extend_map for the rig: the frames are localised against the map (localize(), gate max_tag_rms_px), then
        every id the map does not have is located from the frames that got a pose (locate_tags(), gate max_view_rms_px) ->
        (locate.LocateResult, (n_frames,) CAM_POSE_DTYPE world<-rig).  The record block grows to cover every id seen;
        tag_sizes ({id: size}): the known side of unmapped tags that is not tag_size."""
        from .locate import wanted_records
        o = self._block(obs)
        rec = wanted_records(o, tag_map, tag_sizes)
        poses = self.localize(det, o, rec, tag_size, max_tag_rms_px=max_tag_rms_px)
        return self.locate_tags(det, o, poses, rec, tag_size, max_view_rms_px=max_view_rms_px, min_views=min_views, sigma_px=sigma_px), poses

    def _block(self, obs):
        o = np.asarray(obs)
        if o.dtype != OBS_DTYPE or o.ndim != 3 or o.shape[0] != len(self.cameras):
            raise ValueError("obs must be (%d, n_frames, max_tags) asl_obs records" % len(self.cameras))
        if o.shape[0] * o.shape[2] > MAX_SLOTS:
            raise ValueError("n_cams * max_tags must be <= %d" % MAX_SLOTS)
        return o

    def localize_sequence(self, det, obs, tag_map, tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, seed=None,
                          times=None, huber_px=0.0, with_cov=False):
        """The rig's consecutive frames solved together (Detector.smooth_rig): obs (n_cams, n_frames, max_tags) OBS_DTYPE,
        camera-major -> smooth.SmoothResult with world<-rig for EVERY frame.  seed: localize() of the same obs (None: it runs
        first, and is not kept); times, huber_px, with_cov: as Detector.smooth."""
        r = det.smooth_rig(self._block(obs), tag_map, self.as_records(), tag_size, sigma_px, sigma_rot, sigma_trans, max_iters, seed, None, times,
                           huber_px, with_cov)
        return SmoothResult(r[0], r[1], seed=seed, cov=r[2] if with_cov else None, times=times)

    def localize_sequences(self, det, obs, seq_start, tag_map, tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, seed=None,
                           times=None, huber_px=0.0, with_cov=False):
        """Several sequences of the rig in one call, solved side by side: sequence k is the frames seq_start[k]:seq_start[k + 1]
        of obs (n_seq + 1 offsets from 0 to n_frames) -> [smooth.SmoothResult], each what localize_sequence returns for its
        frames alone."""
        r = det.smooth_rig(self._block(obs), tag_map, self.as_records(), tag_size, sigma_px, sigma_rot, sigma_trans, max_iters, seed, seq_start, times,
                           huber_px, with_cov)
        ss = np.asarray(seq_start, dtype=np.int64).ravel()
        tm = None if times is None else np.asarray(times, dtype=np.float64).ravel()
        return [SmoothResult(r[0][a:b], r[1][k], seed=None if seed is None else np.asarray(seed)[a:b], cov=r[2][a:b] if with_cov else None,
                             times=None if tm is None else tm[a:b]) for k, (a, b) in enumerate(zip(ss[:-1], ss[1:]))]

    def calibrate_mountings(self, det, obs, tag_map, tag_size, max_iters=30, sigma_px=None):
        """The mountings refined jointly with one rig pose per frame (Detector.calibrate_rig, asl_calibrate_rig_batch), this
        rig's mountings the initial ones: obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, of a known tag_map ->
        RigCalibrationResult.  Camera 0's mounting is the gauge and stays; a camera that shares no frame with the cameras
        connected to camera 0 is held (result["cam_status"] 2).  2 to MAX_CALIBRATED_CAMERAS cameras.  sigma_px None or 0: the
        covariances are scaled by the solve's own estimate.  There is no outlier gate: pass clean observations.  The frames
        outside the joint solve (poses status 5) are localised under this rig's mountings: result.rig.localize() re-localises them."""
        if not 2 <= len(self.cameras) <= MAX_CALIBRATED_CAMERAS:
            raise ValueError("calibrate_mountings takes a rig of 2 to %d cameras" % MAX_CALIBRATED_CAMERAS)
        rec, res, cov, poses = det.calibrate_rig(self._block(obs), tag_map, self.as_records(), tag_size, max_iters=max_iters, sigma_px=sigma_px)
        return RigCalibrationResult(Rig.from_records(rec), res, cov, poses)

    @classmethod
    def from_camera_poses(cls, cams, poses_by_cam):
        """The mounting from per-camera localisations of the same frames.  cams: (K, dist) per camera; poses_by_cam:
        per camera an (n_frames,) CAM_POSE_DTYPE array (Detector.localize on that camera's stream).  The rig frame is
        camera 0.  For every frame where camera 0 and camera c both have status 0, E_c(f) = inv(T_wc_c(f)) T_wc_0(f); E_c is
        the rotation nearest to the mean of the R (SVD, det +1) and the mean translation.  The mountings are not refined
        jointly with anything: this is the average of what the single-camera solves imply.  calibrate_mountings() refines
        them jointly, seeded from this average.  Where each camera sees one small tag, a single frame's pose can sit in its
        mirrored minimum and poison the average: each camera's poses from TagDetector.localize_sequence (Detector.smooth) are
        then the better input."""
        poses = [np.asarray(p, dtype=CAM_POSE_DTYPE).ravel() for p in poses_by_cam]
        if len(cams) != len(poses) or not poses or any(len(p) != len(poses[0]) for p in poses):
            raise ValueError("one (K, dist) and one pose array of the same frames per camera")
        out = []
        for c, ((K, dist), p) in enumerate(zip(cams, poses)):
            if c == 0:
                out.append(RigCamera(K, dist, np.eye(4)))
                continue
            both = np.flatnonzero((poses[0]["status"] == 0) & (p["status"] == 0))
            if len(both) == 0:
                raise ValueError("camera %d shares no localised frame with camera 0" % c)
            E = np.array([np.linalg.inv(p["T"][f]) @ poses[0]["T"][f] for f in both])
            U, _, Vt = np.linalg.svd(E[:, :3, :3].mean(axis=0))
            R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, E[:, :3, 3].mean(axis=0)
            out.append(RigCamera(K, dist, T))
        return cls(out)


class RigCalibrationResult:
    """What Rig.calibrate_mountings returns: rig (a new Rig with the refined mountings; the given one where result["status"] is
    not 0), result (RIG_CALIB_RESULT_DTYPE record), cov ((n_cams,) POSE_COV_DTYPE of the mountings, status 1 for camera 0
    and for held cameras) and poses ((n_frames,) CAM_POSE_DTYPE, world<-rig)."""

    def __init__(self, rig, result, cov, poses):
        self.rig, self.result, self.cov, self.poses = rig, result, cov, poses

    @property
    def ok(self):
        return int(self.result["status"]) == 0

    def mounting_std(self):
        """(n_cams, 6): the square roots of the covariance diagonals (rx ry rz in radians, px py pz in map units) of every
        camera's mounting; zeros for a camera without a covariance"""
        return np.sqrt(np.array([np.diag(c) for c in self.cov["cov"]]))

    def save(self, path):
        """Write the result as two files: the rig (Rig.save) at path, the records beside it at path + ".records.npz"."""
        self.rig.save(path)
        np.savez(_records_path(path), result=self.result, cov=self.cov, poses=self.poses)

    @classmethod
    def load(cls, path):
        """The result RigCalibrationResult.save wrote."""
        from ._lib import POSE_COV_DTYPE, RIG_CALIB_RESULT_DTYPE
        rig = Rig.load(path if str(path).endswith(".npz") else str(path) + ".npz")
        with np.load(_records_path(path)) as z:
            return cls(rig, z["result"].astype(RIG_CALIB_RESULT_DTYPE).reshape(()), z["cov"].astype(POSE_COV_DTYPE), z["poses"].astype(CAM_POSE_DTYPE))


def _records_path(path):
    p = str(path)
    return (p[:-4] if p.endswith(".npz") else p) + ".records.npz"
