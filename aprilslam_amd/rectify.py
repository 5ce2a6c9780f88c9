"""Lens rectification ahead of the detector: the geometry a caller needs around `TagDetector(..., rectify=True)`,
`_lib.Detector.rectify` and `_lib.Detector.rectify_frames_device` (asl_rectify_u8 / asl_rectify_frames_device).

The kernel takes every pixel centre of the rectified image through the inverse of the pinhole K_new, the forward
Brown-Conrady model (k1 k2 p1 p2 k3) and the source camera K, and samples the source there.  Detections on a rectified frame
are therefore in rectified pixels, and their camera is K_new without distortion; `distort_points` takes such points back
into the frame the camera delivered, e.g. to draw on it.

A lens no single pinhole holds -- a 150-200 degree fisheye -- is rectified into several rotated pinhole views
(asl_rectify_views_device, `_lib.Detector.rectify_views`): `ViewSet` holds the lens and the views, rectifies frames into
them and hands the views to the rig solvers as what they are, rigidly mounted pinhole cameras with exactly known
mountings (`ViewSet.rig()`), so that a fisheye camera is localised, smoothed and mapped by `rig.Rig` as it stands.

    distort_points      view pixel -> source pixel (the map the kernels sample through), either lens model, any view
    undistort_points    source pixel -> view pixel
    ViewSet             fan(), rig(), rectify(), rectify_device(), observe_device(), save() / load()

Views that overlap show a tag twice, from the same source pixels.  The rig solvers take both slots, but the two are not
independent, so a covariance that counts both is somewhat optimistic.  Views that abut (fan()'s default step) avoid it."""
import numpy as np

from ._lib import LENS_BROWN, LENS_FISHEYE, LENS_MODELS, MAX_VIEWS, OBS_DTYPE, RECTIFY_VIEW_DTYPE
from .rig import ORTHONORMAL_TOL, Rig, RigCamera

INVERSE_STEPS = 30  # fixed-point (Brown) and Newton (fisheye) steps of undistort_points


def _model(model):
    m = LENS_MODELS.get(model, model)
    if m not in (LENS_BROWN, LENS_FISHEYE):
        raise ValueError("model must be 'brown' or 'fisheye'")
    return m


def _lens_coeffs(dist, m):
    d = np.zeros(0) if dist is None else np.asarray(dist, dtype=np.float64).ravel()
    allowed = (0, 4, 5) if m == LENS_BROWN else (0, 4)
    if len(d) not in allowed:
        raise ValueError("dist must hold 0, 4 or 5 coefficients" if m == LENS_BROWN else "a fisheye lens has 0 or 4 coefficients (k1, k2, k3, k4)")
    return list(d) + [0.0] * (allowed[-1] - len(d))


def _rotation(R, what="R"):
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    if R.shape != (3, 3) or not np.all(np.isfinite(R)) or np.abs(R @ R.T - np.eye(3)).max() > ORTHONORMAL_TOL or not np.linalg.det(R) > 0:
        raise ValueError("%s is not a 3x3 rotation" % what)
    return R


def _theta_max(theta_max):
    tm = np.pi if not theta_max else float(theta_max)
    if not 0 < tm <= np.pi:
        raise ValueError("theta_max must lie in (0, pi]")
    return tm


def distort_points(pts, K, dist, K_new=None, R=None, model="brown", theta_max=None):
    """(..., 2) pixel coordinates in the rectified image (pixel (ix, iy) covers [ix, ix+1) x [iy, iy+1)) -> the same points
    in the source image: the map the rectification kernel samples through.  dist: None or 0, 4 or 5 coefficients
    (k1, k2, p1, p2[, k3]); K_new: the pinhole of the rectified image, default K.
    R (source camera <- view) and model ("brown" / "fisheye", dist then k1 k2 k3 k4): the map of a rotated view
    (asl_rectify_views_device); NaN where the kernel writes `fill` because of the lens -- behind the camera under "brown",
    further than theta_max (radians, default pi) from the axis under "fisheye"."""
    p = np.asarray(pts, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    m = _model(model)
    xn = (p[..., 0] - Kn[0, 2]) / Kn[0, 0]
    yn = (p[..., 1] - Kn[1, 2]) / Kn[1, 1]
    if R is None and m == LENS_BROWN:
        return _brown(xn, yn, K, _lens_coeffs(dist, m))
    R = _rotation(R)
    X = R[0, 0] * xn + R[0, 1] * yn + R[0, 2]
    Y = R[1, 0] * xn + R[1, 1] * yn + R[1, 2]
    Z = R[2, 0] * xn + R[2, 1] * yn + R[2, 2]
    return project_rays(np.stack([X, Y, Z], axis=-1), K, dist, m, theta_max)


def _brown(xn, yn, K, coeffs):
    k1, k2, p1, p2, k3 = coeffs
    r2 = xn * xn + yn * yn
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=-1)


def project_rays(rays, K, dist, model="brown", theta_max=None):
    """(..., 3) rays in the source camera's frame -> (..., 2) source pixels under the lens; NaN where the lens has none"""
    d = np.asarray(rays, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    m = _model(model)
    c = _lens_coeffs(dist, m)
    X, Y, Z = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        if m == LENS_BROWN:
            out = _brown(X / Z, Y / Z, K, c)
            gone = Z <= 0
        else:
            k1, k2, k3, k4 = c
            r = np.sqrt(X * X + Y * Y)
            th = np.arctan2(r, Z)
            t2 = th * th
            td = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r == 0, 0.0, td / r)
            out = np.stack([K[0, 0] * (s * X) + K[0, 2], K[1, 1] * (s * Y) + K[1, 2]], axis=-1)
            gone = th > _theta_max(theta_max)
    return np.where(gone[..., None], np.nan, out)


def unproject_points(pts, K, dist, model="brown"):
    """(..., 2) source pixels -> (..., 3) rays in the source camera's frame (unit rays under "fisheye", z = 1 under
    "brown"): the inverse of the lens by INVERSE_STEPS fixed-point / Newton steps"""
    p = np.asarray(pts, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    m = _model(model)
    c = _lens_coeffs(dist, m)
    xd = (p[..., 0] - K[0, 2]) / K[0, 0]
    yd = (p[..., 1] - K[1, 2]) / K[1, 1]
    if m == LENS_BROWN:
        k1, k2, p1, p2, k3 = c
        x, y = xd, yd
        for _ in range(INVERSE_STEPS):
            r2 = x * x + y * y
            rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
            x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
        return np.stack([x, y, np.ones_like(x)], axis=-1)
    k1, k2, k3, k4 = c
    td = np.sqrt(xd * xd + yd * yd)
    th = td
    for _ in range(INVERSE_STEPS):
        t2 = th * th
        f = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
        th = th - f / (1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4))))
    with np.errstate(all="ignore"):
        q = np.where(td == 0, 0.0, np.sin(th) / td)
    return np.stack([q * xd, q * yd, np.cos(th)], axis=-1)


def undistort_points(pts, K, dist, K_new=None, R=None, model="brown"):
    """(..., 2) pixel coordinates in the source image -> the same points in the view (K_new, R) (default K, the identity):
    the inverse of distort_points.  NaN where the ray is behind the view."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kn = K if K_new is None else np.asarray(K_new, dtype=np.float64).reshape(3, 3)
    d = unproject_points(pts, K, dist, model) @ _rotation(R)  # rows d^T R = (R^T d)^T: the rays in the view's frame
    with np.errstate(all="ignore"):
        u = Kn[0, 0] * (d[..., 0] / d[..., 2]) + Kn[0, 2]
        v = Kn[1, 1] * (d[..., 1] / d[..., 2]) + Kn[1, 2]
    return np.where((d[..., 2] > 0)[..., None], np.stack([u, v], axis=-1), np.nan)


def _axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    if axis == "y":   # a positive angle turns the view towards +x: to the right in the image
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    if axis == "x":   # a positive angle turns the view towards +y: down in the image
        return np.array([[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]])
    raise ValueError("axis must be 'x' or 'y'")


class ViewSet:
    """A camera with a lens (K, dist, model) and the rotated pinhole views its frames are rectified into: views is
    [(K_new, R)], R = source camera <- view, all of size = (w_out, h_out).  theta_max (radians, None = pi): fisheye rays
    further from the axis give `fill`."""

    def __init__(self, K, dist, model, views, size, theta_max=None, fill=0):
        self.K = np.array(K, dtype=np.float64)
        if self.K.shape != (3, 3) or not np.all(np.isfinite(self.K)):
            raise ValueError("K must be a finite 3x3 matrix")
        self.model = _model(model)
        self.dist = np.array([] if dist is None else dist, dtype=np.float64).ravel()
        _lens_coeffs(self.dist, self.model)
        self.views = []
        for k, (K_new, R) in enumerate(views):
            Kn = np.array(K_new, dtype=np.float64)
            if Kn.shape != (3, 3) or not np.all(np.isfinite(Kn)) or not (Kn[0, 0] > 0 and Kn[1, 1] > 0):
                raise ValueError("view %d: K_new must be a finite 3x3 matrix with positive focal lengths" % k)
            self.views.append((Kn, _rotation(R, "view %d: R" % k)))
        if not 1 <= len(self.views) <= MAX_VIEWS:
            raise ValueError("a ViewSet has 1 to %d views" % MAX_VIEWS)
        self.size = (int(size[0]), int(size[1]))
        self.theta_max = _theta_max(theta_max)
        self.fill = int(fill)
        self._frames = None  # rectify_device / observe_device without a destination: the views on the device, grown on demand
        self._obs = None

    def __len__(self):
        return len(self.views)

    @classmethod
    def fan(cls, K, dist, model, n_views, hfov_deg, size, step_deg=None, axis="y", theta_max=None, fill=0):
        """n_views equal pinholes of hfov_deg (along the fan) turned about the source camera's `axis` ("y": side by side, the
        field of view horizontal; "x": one above the other, the field of view vertical), centred on the optical axis,
        step_deg apart (default hfov_deg: the views abut).  Square pixels, the principal point in the middle."""
        w, h = int(size[0]), int(size[1])
        step = float(hfov_deg if step_deg is None else step_deg)
        if not 0 < hfov_deg < 180:
            raise ValueError("hfov_deg must lie in (0, 180)")
        f = 0.5 * (w if axis == "y" else h) / np.tan(np.radians(0.5 * hfov_deg))
        K_new = np.array([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]])
        angles = [np.radians(step * (k - 0.5 * (n_views - 1))) for k in range(n_views)]
        return cls(K, dist, model, [(K_new, _axis_rotation(axis, a)) for a in angles], size, theta_max=theta_max, fill=fill)

    def records(self):
        """(n_views,) RECTIFY_VIEW_DTYPE: the table the library reads"""
        rec = np.zeros(len(self.views), dtype=RECTIFY_VIEW_DTYPE)
        for k, (Kn, R) in enumerate(self.views):
            rec["K"][k], rec["R"][k] = Kn, R
        return rec

    def rig(self):
        """The views as the rig they are: RigCamera(K_new, no lens, camera<-rig = [R^T | 0]); the rig frame is the source
        camera's frame, so a pose world<-rig is the pose of the camera itself."""
        cams = []
        for Kn, R in self.views:
            T = np.eye(4)
            T[:3, :3] = R.T
            cams.append(RigCamera(Kn, None, T))
        return Rig(cams)

    def distort_points(self, view, pts):
        """pixels of view `view` -> source pixels"""
        Kn, R = self.views[view]
        return distort_points(pts, self.K, self.dist, Kn, R, self.model, self.theta_max)

    def undistort_points(self, view, pts):
        """source pixels -> pixels of view `view` (NaN behind it)"""
        Kn, R = self.views[view]
        return undistort_points(pts, self.K, self.dist, Kn, R, self.model)

    def rectify(self, det, image):
        """one host image of the camera -> (n_views, h_out, w_out) gray (asl_rectify_views_u8 on det, a _lib.Detector)"""
        return det.rectify_views(image, self.K, self.dist, self.records(), model=self.model, size=self.size, theta_max=self.theta_max,
                                 fill=self.fill)

    def rectify_device(self, det, src_ptr, n_frames, channels, w, h, dst_ptr=None, stream=0, **pitches):
        """n_frames frames at the device address src_ptr -> the views, view-major, at dst_ptr (asl_rectify_views_device;
        pitches: stride, frame_pitch, stride_out, frame_pitch_out).  Without dst_ptr the views go into a buffer this
        ViewSet keeps; returns the destination's address.  Enqueued on `stream`, no wait."""
        if dst_ptr is None:
            import torch
            need = len(self.views) * int(n_frames) * self.size[0] * self.size[1]
            if pitches.get("stride_out") or pitches.get("frame_pitch_out"):
                raise ValueError("output pitches need a dst_ptr")
            if self._frames is None or self._frames.numel() < need:
                self._frames = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % det.device)
            dst_ptr = self._frames.data_ptr()
        det.rectify_views_device(src_ptr, n_frames, channels, w, h, dst_ptr, self.K, self.dist, self.records(), model=self.model,
                                 width_out=self.size[0], height_out=self.size[1], theta_max=self.theta_max, fill=self.fill, stream=stream, **pitches)
        return dst_ptr

    def observe_device(self, det, src_ptr, n_frames, channels, w, h, tag_size, max_tags, stream=0, **pitches):
        """Frames on the device -> (n_views, n_frames, max_tags) OBS_DTYPE, the camera-major block Rig.localize,
        localize_sequence, build_map and locate_tags of rig() take.  The frames are rectified into the views; each view's
        frames are one batch for the detector, submitted with that view's K_new and no lens, packed into the view's slice
        of one device block and collected; the block comes back in one copy."""
        import torch
        wo, ho = self.size
        n_frames, max_tags = int(n_frames), int(max_tags)
        frames = self.rectify_device(det, src_ptr, n_frames, channels, w, h, stream=stream, **pitches)
        need = len(self.views) * n_frames * max_tags * OBS_DTYPE.itemsize
        if self._obs is None or self._obs.numel() < need:
            self._obs = torch.empty(need, dtype=torch.uint8, device="cuda:%d" % det.device)
        for v, (Kn, _) in enumerate(self.views):
            det.submit_device(frames + v * n_frames * wo * ho, n_frames, 1, wo, ho, stream=stream, K=Kn, dist=np.zeros(0), tag_size=tag_size)
            det.pack_observations_device(self._obs.data_ptr() + v * n_frames * max_tags * OBS_DTYPE.itemsize, max_tags, stream=stream)
            det.collect()
        if stream:
            torch.cuda.ExternalStream(int(stream)).synchronize()
        else:
            torch.cuda.synchronize(det.device)
        return self._obs[:need].cpu().numpy().view(OBS_DTYPE).reshape(len(self.views), n_frames, max_tags).copy()

    def save(self, path):
        """Write the set to an .npz file: K, dist, model, view_K (n, 3, 3), view_R (n, 3, 3), size, theta_max, fill."""
        np.savez(path, K=self.K, dist=self.dist, model=np.int64(self.model), view_K=np.array([v[0] for v in self.views]),
                 view_R=np.array([v[1] for v in self.views]), size=np.array(self.size, dtype=np.int64), theta_max=np.float64(self.theta_max),
                 fill=np.int64(self.fill))

    @classmethod
    def load(cls, path):
        """The set ViewSet.save wrote."""
        with np.load(path) as z:
            vk, vr = z["view_K"], z["view_R"]
            if vk.ndim != 3 or vk.shape != vr.shape or vk.shape[1:] != (3, 3):
                raise ValueError("%s is not a saved ViewSet" % path)
            return cls(z["K"], z["dist"], int(z["model"]), list(zip(vk, vr)), tuple(int(s) for s in z["size"]), theta_max=float(z["theta_max"]),
                       fill=int(z["fill"]))
