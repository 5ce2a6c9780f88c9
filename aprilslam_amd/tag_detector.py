"""`TagDetector`: host-side mirror of reference src/detection/tag_detector.py:14-88.

Same constructor, methods, argument meaning and return shapes.  The three native calls of
the reference are replaced by the C ABI of libaprilslam.so:
    cv2.cvtColor(BGR2GRAY) + apriltag.detect   -> asl_detect_bgr_u8   (gray conversion fused)
    cv2.solvePnP + cv2.Rodrigues               -> asl_solve_pnp_batch
`detect_batch` / `get_poses` are the batched forms the GPU wants; `detect` / `get_pose` keep
the reference's one-frame / one-tag call surface.
"""
import numpy as np

from . import _lib
from .apriltag import apriltag


def rodrigues(rvec):
    """cv2.Rodrigues(rvec)[0]: rotation vector -> 3x3 matrix (host, float64)."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    theta = float(np.sqrt(r @ r))
    if theta < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / theta
    c, s = np.cos(theta), np.sin(theta)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return c * np.eye(3) + (1 - c) * np.outer(k, k) + s * Kx


class TagDetector:
    """Handles AprilTag detection and pose estimation (GPU-backed)."""

    def __init__(self, camera_params, tag_type="tagStandard41h12", tag_size=0.06, device=0, id_limit=None, quad_sigma=0.0,
                 rectify=False, rectified_K=None, lens_model="brown"):
        """tag_type: a family's name, or a list of registered names (one detector for all; ids are then global and the
        detections carry 'family' and 'local_id', see apriltag).
        quad_sigma: the detector's blur (> 0) or sharpening (< 0) of the decimated image; the reference leaves it 0.
        rectify: take every frame through the lens rectification first (asl_rectify_u8 / asl_rectify_frames_device with
        camera_params as the source camera), into a buffer this detector owns, and detect on the gray result -- for a lens
        strong enough to bend a tag's edges.  DETECTIONS ARE THEN IN RECTIFIED PIXELS (rectify.distort_points takes them back
        into the frame the camera delivered), and every pose call uses the pinhole rectified_K (default: the camera matrix)
        with no distortion.  False, the default, is the path without the keyword.
        lens_model: "brown" (dist_coeffs k1 k2 p1 p2 [k3]) or "fisheye" (dist_coeffs k1 k2 k3 k4, the cv2.fisheye model).  A
        fisheye needs rectify=True, since no pose solver takes that lens: the frames go through asl_rectify_views_u8 /
        asl_rectify_views_device into the one view rectified_K with R the identity.  A field of view no single pinhole
        holds takes several views: rectify.ViewSet.  A fisheye's K and coefficients come from
        calibrate(.., lens_model="fisheye") of a detector on the raw frames."""
        if lens_model not in ("brown", "fisheye"):
            raise ValueError("lens_model must be 'brown' or 'fisheye'")
        if lens_model == "fisheye" and not rectify:
            raise ValueError("a fisheye lens needs rectify=True: no solver takes that lens")
        self.lens_model = lens_model
        self.detector = apriltag(tag_type, blur=quad_sigma, device=device, id_limit=id_limit)
        self.tag_size = tag_size
        self.camera_matrix = camera_params['camera_matrix']
        self.dist_coeffs = camera_params['dist_coeffs']
        self.rectify = bool(rectify)
        self.rectified_K = None
        if self.rectify:
            self.rectified_K = np.array(self.camera_matrix if rectified_K is None else rectified_K, dtype=np.float64).reshape(3, 3)
        elif rectified_K is not None:
            raise ValueError("rectified_K needs rectify=True")
        self._device = int(device)
        self._rect_buf = None  # detect_batch_device: the rectified frames on the device, grown on demand

    # -- reference call surface ------------------------------------------------------
    def detect(self, image):
        """BGR (H,W,3) uint8 image -> list of detection dicts sorted by id (tag_detector.py:23-28)."""
        a = np.asarray(image)
        if a.ndim == 2:
            return sorted(self.detector.detect(self._rectified_host(a) if self.rectify else a), key=lambda d: d['id'])
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError("expected an (H, W, 3) uint8 BGR image")
        if self.rectify:
            a = self._rectified_host(a)  # (H, W) gray, in rectified pixels
        # the poses are solved in the same device submission (asl_detect_batch_pose_u8) and ride along under a
        # private key, so that get_pose() of these detections needs no second trip to the GPU; the arithmetic is
        # the one get_pose() does on its own (float32-rounded corners -> asl_solve_pnp_batch), bit for bit
        dets, poses, _ = self.detector._det.detect_host(np.ascontiguousarray(a), K=self._K(), dist=self._dist(),
                                                        tag_size=self.tag_size)
        out = [dict({"hamming": int(d["hamming"]), "margin": float(d["margin"]), "id": int(d["id"]),
                     "center": np.array(d["center"]), "lb-rb-rt-lt": np.array(d["corners"]),
                     "_pose": (np.array(d["corners"]), self._pose_key(), bool(p["ok"]), np.array(p["rvec"]), np.array(p["tvec"]))},
                    **self.detector.family_keys(int(d["id"])))  # a list of families: 'family' and 'local_id' as well
               for d, p in zip(dets, poses)]
        return sorted(out, key=lambda d: d['id'])

    def get_pose(self, detection):
        """(retval, rvec(3,1), tvec(3,1), T 4x4) of one detection (tag_detector.py:30-43)."""
        cached = detection.get('_pose') if isinstance(detection, dict) else None
        if cached is not None and cached[1] == self._pose_key() and np.array_equal(cached[0], detection['lb-rb-rt-lt']):
            rv, tv = cached[3].reshape(3, 1).copy(), cached[4].reshape(3, 1).copy()
            return cached[2], rv, tv, self.transformation(rv, tv)
        corners = np.array(detection['lb-rb-rt-lt'], dtype=np.float32)
        rvec, tvec, _, ok = self.detector._det.solve_pnp(corners[None], self._K(), self._dist(), self.tag_size)
        rv, tv = rvec[0].reshape(3, 1), tvec[0].reshape(3, 1)
        return bool(ok[0]), rv, tv, self.transformation(rv, tv)

    def transformation(self, rvec, tvec):
        T = np.eye(4)
        T[:3, :3] = rodrigues(rvec)
        T[:3, 3] = np.asarray(tvec, dtype=np.float64).flatten()
        return T

    def euler_angles(self, rvec):
        """[yaw, pitch, roll] in degrees, the reference's convention (tag_detector.py:54-69)."""
        R = rodrigues(rvec)
        sy = np.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2)
        if sy >= 1e-6:
            yaw = np.arctan2(R[0, 2], R[2, 2])
            pitch = np.arctan2(-R[1, 2], sy)
            roll = np.arctan2(R[1, 0], R[1, 1])
        else:
            yaw = np.arctan2(-R[2, 0], R[0, 0])
            pitch = np.arctan2(-R[1, 2], sy)
            roll = 0
        return np.degrees([yaw, pitch, roll])

    def distance(self, tvec):
        return np.linalg.norm(tvec)

    def draw(self, rvec, tvec, corners, image, tag_id):
        """Overlay drawing needs OpenCV's GUI primitives; without cv2 the image is returned as is."""
        try:
            import cv2  # noqa: F401
        except ImportError:
            return image
        for i in range(4):
            p1 = tuple(map(int, corners[i]))
            p2 = tuple(map(int, corners[(i + 1) % 4]))
            cv2.line(image, p1, p2, (0, 255, 0), 2)
        yaw, pitch, roll = self.euler_angles(rvec)
        cv2.putText(image, f'ID: {tag_id}, Dist: {self.distance(tvec):.1f} units', (p1[0], p1[1] - 20),
                    cv2.FONT_HERSHEY_SIMPLEX, 0.5, (0, 165, 255), 2)
        cv2.putText(image, f'Yaw: {yaw:.1f}, Pitch: {pitch:.1f}, Roll: {roll:.1f}', (p1[0], p1[1] - 40),
                    cv2.FONT_HERSHEY_SIMPLEX, 0.5, (0, 165, 255), 2)
        return image

    # -- batched forms ------------------------------------------------------------------
    def _pose_key(self):
        """what a cached pose depends on besides the corners: tag size and intrinsics, by value"""
        return (float(self.tag_size), np.asarray(self._K(), dtype=np.float64).tobytes(), self._dist().tobytes())

    def _lens(self):
        """the camera's own lens coefficients"""
        d = np.asarray(self.dist_coeffs, dtype=np.float64).ravel()
        if self.lens_model == "fisheye":
            if len(d) not in (0, 4):
                raise ValueError("a fisheye's dist_coeffs hold 0 or 4 values")
        elif len(d) not in (0, 4, 5):
            raise ValueError("dist_coeffs must hold 0, 4 or 5 values")
        return d

    def _K(self):
        """the camera matrix of the pixels the detections are in"""
        return self.rectified_K if self.rectify else self.camera_matrix

    def _dist(self):
        """the lens of the pixels the detections are in: none once the frames are rectified"""
        return np.zeros(0) if self.rectify else self._lens()

    def _rectified_host(self, image):
        """one host image, gray or BGR -> its rectified gray image (asl_rectify_u8; a fisheye: asl_rectify_views_u8)"""
        if self.lens_model == "fisheye":
            return self.detector._det.rectify_views(image, self.camera_matrix, self._lens(), [(self.rectified_K, None)], model="fisheye")[0]
        return self.detector._det.rectify(image, self.camera_matrix, self._lens(), K_new=self.rectified_K)

    def get_poses(self, detections):
        """PnP for many detections in one launch: returns (ok[N], rvec[N,3], tvec[N,3], T[N,4,4])."""
        if not detections:
            return np.zeros(0, bool), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4, 4))
        c = np.stack([np.asarray(d['lb-rb-rt-lt'], dtype=np.float32) for d in detections])
        rvec, tvec, T, ok = self.detector._det.solve_pnp(c, self._K(), self._dist(), self.tag_size)
        return ok, rvec, tvec, T

    def get_poses_cov(self, detections, sigma_px=0.0):
        """get_poses with each pose's covariance (asl_solve_pnp_cov_batch): (ok[N], rvec[N,3], tvec[N,3], T[N,4,4],
        cov[N] POSE_COV_DTYPE), camera<-tag, (rx ry rz | tvec); sigma_px = 0 estimates the corner sigma from the tag's own
        8 residuals (2 degrees of freedom: a given sigma_px is the better choice).  A pose that is not ok has status 1."""
        ok, rvec, tvec, T = self.get_poses(detections)
        if not len(ok):
            return ok, rvec, tvec, T, np.zeros(0, dtype=_lib.POSE_COV_DTYPE)
        c = np.stack([np.asarray(d['lb-rb-rt-lt'], dtype=np.float32) for d in detections])
        Tc = np.where(np.asarray(ok, dtype=bool)[:, None, None], T, np.nan)
        cov = self.detector._det.pose_cov(c, Tc, self._K(), self._dist(), self.tag_size, sigma_px)
        return ok, rvec, tvec, T, cov

    # -- camera pose from every visible tag against a known map (asl_localize_batch) ---------------------------------
    def localize(self, detections, tag_map, max_tag_rms_px=0.0, with_cov=False, sigma_px=0.0, map_cov=None):
        """One frame's detection dicts (as detect() returns them) -> the camera pose from all mapped tags at once:
        {"ok", "T" world<-camera 4x4, "rms_px", "n_tags", "n_rejected", "status"}.  The poses detect() solved in its own
        submission are reused; detections without one get their PnP first (one launch).  max_tag_rms_px > 0 drops tags
        whose own corner RMS exceeds it (moved or mis-identified tags) and solves again.  with_cov adds "cov" (6x6,
        rotation about the world axes | camera position, zeros unless "cov_status" is 0) and "sigma_px", the corner sigma
        that scaled it: the given one, or for 0 the solve's own estimate (localize.pose_std reads the std off it).
        A tag with a size of its own in tag_map (TagMap.set_size) is solved at it, here and in localize_batch /
        localize_sequence / localize_sequences; this detector's tag_size is the size of the others.
        map_cov (with with_cov; a mapping.MapCovariance, e.g. build_map(with_cov=True).cov): the uncertainty of the map's
        tags is carried into "cov" (asl_localize_mapcov_batch); "cov_status" 3: map_cov does not fit the map."""
        if map_cov is not None and not with_cov:
            raise ValueError("map_cov needs with_cov=True")
        dets = list(detections)
        if len(dets) > 256:
            raise ValueError("at most 256 detections per frame")
        obs = np.zeros((1, max(1, len(dets))), dtype=_lib.OBS_DTYPE)
        obs["id"] = -1
        Ts = [None] * len(dets)
        oks = [False] * len(dets)
        missing = []
        for k, d in enumerate(dets):
            cached = d.get('_pose') if isinstance(d, dict) else None
            if cached is not None and cached[1] == self._pose_key() and np.array_equal(cached[0], d['lb-rb-rt-lt']):
                oks[k], Ts[k] = cached[2], self.transformation(cached[3], cached[4])
            else:
                missing.append(k)
        if missing:
            ok, _, _, T = self.get_poses([dets[k] for k in missing])
            for j, k in enumerate(missing):
                oks[k], Ts[k] = bool(ok[j]), T[j]
        for k, d in enumerate(dets):
            obs["id"][0, k] = int(d['id'])
            obs["flags"][0, k] = 1 | (2 if oks[k] else 0)
            obs["corners"][0, k] = np.asarray(d['lb-rb-rt-lt'], dtype=np.float32).reshape(8)
            obs["T"][0, k] = np.asarray(Ts[k], dtype=np.float64).reshape(16)[:12]
        res = self.detector._det.localize(obs, tag_map, self._K(), self._dist(), self.tag_size, max_tag_rms_px,
                                          sigma_px=float(sigma_px) if with_cov else None, map_cov=map_cov)
        r = (res[0] if with_cov else res)[0]
        out = {"ok": int(r["status"]) == 0, "T": np.array(r["T"]), "rms_px": float(r["rms_px"]), "n_tags": int(r["n_tags"]),
               "n_rejected": int(r["n_rejected"]), "status": int(r["status"])}
        if with_cov:
            c = res[1][0]
            out.update(cov=np.array(c["cov"]), sigma_px=float(c["sigma_px"]), cov_status=int(c["status"]))
        return out

    def localize_batch(self, dets, poses, n_per_frame, tag_map, max_tag_rms_px=0.0, max_tags=None, with_cov=False, sigma_px=0.0):
        """The structured arrays detect_host / collect return (detections in (frame, id) order, their poses, the count per
        frame) -> one CAM_POSE_DTYPE record per frame.  max_tags: slots per frame (default: the most detections of a frame).
        with_cov: (poses, one POSE_COV_DTYPE record per frame) instead."""
        from .dist import pack_observations
        npf = np.asarray(n_per_frame, dtype=np.int64)
        mt = int(max_tags) if max_tags is not None else max(1, int(npf.max()) if len(npf) else 1)
        obs = pack_observations(dets, poses, npf, mt)
        return self.detector._det.localize(obs, tag_map, self._K(), self._dist(), self.tag_size, max_tag_rms_px,
                                           sigma_px=float(sigma_px) if with_cov else None)

    def localize_bundles(self, dets, poses, n_per_frame, bundles, ref=None, max_tag_rms_px=0.0, with_cov=False, sigma_px=0.0, max_tags=None):
        """localize_batch against every bundle of a bundles.BundleSet at once (asl_localize_bundles_batch): several rigid
        objects that each carry a few tags, every one posed in every frame -> bundles.BundleResult with T[f, b] =
        bundle_b<-camera (status 1 where the frame sees no tag of the bundle) and, with_cov, the covariances.  ref (a
        position or a name): (result, result.relative(ref)) instead, the second (n_frames, n_bundles) BUNDLE_REL_DTYPE with
        T = ref<-bundle and its covariance."""
        from .bundles import BundleResult
        from .dist import pack_observations
        npf = np.asarray(n_per_frame, dtype=np.int64)
        mt = int(max_tags) if max_tags is not None else max(1, int(npf.max()) if len(npf) else 1)
        obs = pack_observations(dets, poses, npf, mt)
        det = self.detector._det
        got = det.localize_bundles(obs, bundles, self._K(), self._dist(), self.tag_size, max_tag_rms_px, float(sigma_px) if with_cov else None)
        res = BundleResult(got[0], got[1], bundles, det) if with_cov else BundleResult(got, None, bundles, det)
        return res if ref is None else (res, res.relative(ref))

    def localize_sequence(self, dets, poses, n_per_frame, tag_map, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20,
                          max_tags=None, with_cov=False, huber_px=0.0, times=None):
        """The structured arrays detect_host / collect return for one camera's CONSECUTIVE frames -> smooth.SmoothResult: a
        world<-camera pose for every frame, the frames solved together with a random-walk motion prior (sigma_rot rad and
        sigma_trans scene units per frame step) next to the corners (sigma_px).  Packs, localises every frame on its own
        (the seed, kept in the result) and smooths (asl_smooth_batch).  with_cov: asl_smooth_cov_batch, and the result
        carries every pose's covariance under the three sigmas (.cov, .cov_status, .pose_std()), the frames carried by the
        prior alone included.  huber_px > 0: a Huber loss of that many pixels on every corner's residual
        (asl_smooth_robust_sequences_batch), for a slipped corner or a slot with another tag's corners; the result's .n_soft
        and .soft say which slots and frames it down-weighted.  Its linear tail needs more trials: raise max_iters.
        times: one strictly increasing time per frame, any unit (asl_smooth_timed_sequences_batch): sigma_rot and sigma_trans
        are then per unit of that time, so frames may be dropped or unevenly spaced; the result keeps them (.times) and
        .pose_at(t) gives the pose between two frames.  Bad times: the result's status is 4, no error."""
        from .dist import pack_observations
        from .smooth import SmoothResult
        npf = np.asarray(n_per_frame, dtype=np.int64)
        mt = int(max_tags) if max_tags is not None else max(1, min(256, int(npf.max()) if len(npf) else 1))
        obs = pack_observations(dets, poses, npf, mt)
        det = self.detector._det
        seed = det.localize(obs, tag_map, self._K(), self._dist(), self.tag_size)
        got = det.smooth(obs, tag_map, self._K(), self._dist(), self.tag_size, sigma_px=sigma_px, sigma_rot=sigma_rot,
                         sigma_trans=sigma_trans, max_iters=max_iters, seed=seed, with_cov=with_cov, huber_px=huber_px,
                         times=times)
        return SmoothResult(got[0], got[1], seed, got[2] if with_cov else None, times)

    def localize_sequences(self, sequences, tag_map, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, max_tags=None,
                           with_cov=False, huber_px=0.0):
        """localize_sequence for several sequences in one call: `sequences` is a list of (dets, poses, n_per_frame) triples (or
        4-tuples with the sequence's frame times last; where some have them, a sequence without gets its frame indices) as
        detect_host / collect return them, each one camera's consecutive frames (different cameras, recordings, or the pieces
        of a recording cut where the camera was off) -> a list of smooth.SmoothResult, one per sequence, each what
        localize_sequence returns for it alone at the same max_tags.  Packs them end to end with one common max_tags,
        localises every frame once (the seeds, kept in the results) and smooths all sequences side by side
        (asl_smooth_sequences_batch): no term links two sequences.  huber_px as in localize_sequence, the same for all."""
        from .dist import pack_observations
        from .smooth import SmoothResult
        if not len(sequences):
            return []
        npfs = [np.asarray(s[2], dtype=np.int64) for s in sequences]
        if any(len(n) == 0 for n in npfs):
            raise ValueError("every sequence needs at least one frame")
        mt = int(max_tags) if max_tags is not None else max(1, min(256, max(int(n.max()) for n in npfs)))
        obs = np.concatenate([pack_observations(s[0], s[1], n, mt) for s, n in zip(sequences, npfs)])
        start = np.concatenate([[0], np.cumsum([len(n) for n in npfs])])
        tms = [np.asarray(s[3], dtype=np.float64).ravel() if len(s) > 3 and s[3] is not None else None for s in sequences]
        if any(t is not None and len(t) != len(n) for t, n in zip(tms, npfs)):
            raise ValueError("a sequence's times must hold one value per frame")
        timed = any(t is not None for t in tms)
        times = np.concatenate([np.arange(len(n), dtype=np.float64) if t is None else t for t, n in zip(tms, npfs)]) if timed else None
        det = self.detector._det
        seed = det.localize(obs, tag_map, self._K(), self._dist(), self.tag_size)
        got = det.smooth_sequences(obs, start, tag_map, self._K(), self._dist(), self.tag_size, sigma_px=sigma_px, sigma_rot=sigma_rot,
                                   sigma_trans=sigma_trans, max_iters=max_iters, seed=seed, with_cov=with_cov, huber_px=huber_px,
                                   times=times)
        return [SmoothResult(got[0][a:b], got[1][k], seed[a:b], got[2][a:b] if with_cov else None, tms[k])
                for k, (a, b) in enumerate(zip(start[:-1], start[1:]))]

    # -- camera calibration from frames of a known target (asl_calibrate_batch) ------------------------------------------
    def calibrate(self, frames, tag_map, n_dist=5, K_init=None, flags=0, max_iters=30, lens_model="brown"):
        """Host frames ((n, H, W, 3) BGR or (n, H, W) gray uint8, or a list of them) that see the target tag_map (a
        localize.TagMap, e.g. TagMap.grid) -> calibrate.CalibrationResult: K, dist (n_dist coefficients), std, per-frame
        poses.  Detect, pack (asl_obs records) and calibrate; this detector's own camera model is not used.  Pass the
        result's camera_params to a TagDetector afterwards.  The target may mix tag sizes (TagMap.set_size); this detector's
        tag_size is the size of the tags that have none of their own.
        lens_model "fisheye" (n_dist 0 or 4: k1 k2 k3 k4): the frames are the fisheye's RAW frames, detected as they are --
        tags out to some 75 degrees off axis are found there -- by a detector made with rectify=False; the result goes to
        TagDetector(cr.camera_params, lens_model="fisheye", rectify=True) or cr.view_set(..)."""
        from .calibrate import CalibrationResult
        from .dist import pack_observations
        if self.rectify:
            raise ValueError("calibrate needs the raw corners: use a TagDetector with rectify=False")
        a = np.ascontiguousarray(np.stack(frames) if isinstance(frames, (list, tuple)) else frames)
        if a.ndim not in (3, 4) or a.dtype != np.uint8:
            raise ValueError("frames must be (n, H, W[, 3]) uint8")
        height, width = a.shape[1], a.shape[2]
        dets, npf = self.detector._det.detect_host(a, channels=1 if a.ndim == 3 else None)
        npf = np.asarray(npf, dtype=np.int64)
        mt = max(1, min(256, int(npf.max()) if len(npf) else 1))
        obs = pack_observations(dets, np.zeros(len(dets), dtype=_lib.POSE_DTYPE), npf, mt)  # the calibration reads no PnP pose
        if lens_model not in ("brown", "fisheye"):
            raise ValueError("lens_model must be 'brown' or 'fisheye'")
        res, cam = self.detector._det.calibrate(obs, tag_map, self.tag_size, width, height, K_init=K_init, n_dist=n_dist, flags=flags,
                                                max_iters=max_iters, model=None if lens_model == "brown" else lens_model)
        return CalibrationResult(res, cam, n_dist, lens_model)

    def build_map(self, frames, world_id=None, max_iters=30, with_std=True, huber_px=0.0, tag_sizes=None, with_cov=False):
        """Host frames ((n, H, W, 3) BGR or (n, H, W) gray uint8, or a list of them) that see an unknown set of tags ->
        mapping.MapResult: the tags' world<-tag poses (tag_map, world tag world_id, default the lowest id seen), every
        frame's camera pose and a per-tag std.  Detect with this detector's camera model and tag size, pack (asl_obs
        records) and map (asl_map_batch).  huber_px > 0: a Huber loss of that many pixels on every corner residual of
        the joint solve (asl_map_robust_batch), so that a slipped corner or a mis-decoded id is down-weighted instead
        of bending the map; the result then has n_soft, slot_weight and soft_slots().  tag_sizes ({id: size}, or an
        array indexed by id that covers every id seen): tags whose side is not the detector's tag_size (0, or an id
        not named: tag_size), each solved at its own (asl_map_sized_batch); result.tag_map carries the sizes, so that
        localize() and localize_sequence() against it, or against the file tag_map.save() writes, honour them.
        with_cov: the joint covariance of the mapped tags as result.cov, a mapping.MapCovariance (asl_mapcov_batch)."""
        from .dist import pack_observations
        from .mapping import MapResult
        if self.camera_matrix is None:
            raise ValueError("build_map needs the detector's camera parameters")
        a = np.ascontiguousarray(np.stack(frames) if isinstance(frames, (list, tuple)) else frames)
        if a.ndim not in (3, 4) or a.dtype != np.uint8:
            raise ValueError("frames must be (n, H, W[, 3]) uint8")
        if self.rectify:
            a = np.stack([self._rectified_host(f) for f in a])
        dist = self._dist()
        dets, poses, npf = self.detector._det.detect_host(a, channels=1 if a.ndim == 3 else None, K=self._K(), dist=dist,
                                                          tag_size=self.tag_size)
        npf = np.asarray(npf, dtype=np.int64)
        mt = max(1, min(256, int(npf.max()) if len(npf) else 1))
        obs = pack_observations(dets, poses, npf, mt)
        n_ids = int(max(1, obs["id"].max() + 1 if obs.size else 1))
        if tag_sizes is not None and not isinstance(tag_sizes, dict):
            table = np.asarray(tag_sizes, dtype=np.float32).ravel()
            if len(table) < n_ids:
                raise ValueError("tag_sizes has %d entries; the frames hold ids up to %d" % (len(table), n_ids - 1))
            tag_sizes = table[:n_ids]
        out = self.detector._det.build_map(obs, n_ids, self._K(), dist, self.tag_size, world_id=-1 if world_id is None else int(world_id),
                                           max_iters=max_iters, with_std=with_std, huber_px=huber_px, with_slot_weight=bool(huber_px),
                                           tag_sizes=tag_sizes, with_cov=with_cov)
        return MapResult.from_call(out, slot_ids=obs["id"] if huber_px else None, with_cov=with_cov)

    def extend_map(self, frames_or_obs, tag_map, tag_sizes=None, max_view_rms_px=0.0, min_views=2, sigma_px=None, max_tag_rms_px=0.0):
        """Frames that see tags of tag_map (a localize.TagMap) and tags it does not have -> (locate.LocateResult, one
        CAM_POSE_DTYPE record per frame): the frames are localised against the map and every unmapped tag is located from
        the frames that got a pose, the cameras held fixed (asl_locate_tags_batch).  The known tags keep their poses.
        frames_or_obs: host frames as build_map takes them, or an (n_frames, max_tags) OBS_DTYPE block.  tag_sizes
        ({id: size}): unmapped tags whose side is not the detector's tag_size.  max_view_rms_px gates single views of a
        tag, max_tag_rms_px the tags of a frame; sigma_px not None adds the located tags' covariances.  The frame poses
        are taken as exact: this is not a joint refinement of cameras and new tags."""
        from .dist import pack_observations
        from .locate import extend_map
        if self.camera_matrix is None:
            raise ValueError("extend_map needs the detector's camera parameters")
        a = frames_or_obs
        if not (isinstance(a, np.ndarray) and a.dtype == _lib.OBS_DTYPE):
            a = np.ascontiguousarray(np.stack(a) if isinstance(a, (list, tuple)) else a)
            if a.ndim not in (3, 4) or a.dtype != np.uint8:
                raise ValueError("frames must be (n, H, W[, 3]) uint8, or an OBS_DTYPE block")
            if self.rectify:
                a = np.stack([self._rectified_host(f) for f in a])
            dets, poses, npf = self.detector._det.detect_host(a, channels=1 if a.ndim == 3 else None, K=self._K(), dist=self._dist(),
                                                              tag_size=self.tag_size)
            npf = np.asarray(npf, dtype=np.int64)
            a = pack_observations(dets, poses, npf, max(1, min(256, int(npf.max()) if len(npf) else 1)))
        return extend_map(self.detector._det, a, tag_map, self._K(), self._dist(), self.tag_size, tag_sizes=tag_sizes,
                          max_view_rms_px=max_view_rms_px, min_views=min_views, sigma_px=sigma_px, max_tag_rms_px=max_tag_rms_px)

    def detect_batch_device(self, data_ptr, n_frames, channels, width, height, with_pose=True, stream=0, **kw):
        """Frames resident in HBM -> (dets, poses, n_per_frame) structured arrays (see _lib).  With rectify the frames are
        rectified on `stream` first, device to device, and the detections are in rectified pixels."""
        if self.rectify:
            import torch
            need = int(n_frames) * int(width) * int(height)
            if self._rect_buf is None or self._rect_buf.numel() < need:
                self._rect_buf = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % self._device)
            pitches = dict(stride=kw.pop("stride", None), frame_pitch=kw.pop("frame_pitch", None), stream=stream)
            if self.lens_model == "fisheye":
                self.detector._det.rectify_views_device(data_ptr, n_frames, channels, width, height, self._rect_buf.data_ptr(), self.camera_matrix,
                                                        self._lens(), [(self.rectified_K, None)], model="fisheye", **pitches)
            else:
                self.detector._det.rectify_frames_device(data_ptr, n_frames, channels, width, height, self._rect_buf.data_ptr(),
                                                         self.camera_matrix, self._lens(), K_new=self.rectified_K, **pitches)
            data_ptr, channels = self._rect_buf.data_ptr(), 1
        K = self._K() if with_pose else None
        return self.detector._det.detect_device(data_ptr, n_frames, channels, width, height, stream=stream, K=K,
                                                dist=self._dist(), tag_size=self.tag_size, **kw)
