"""Camera calibration from tag observations (asl_calibrate_batch / asl_calibrate_frames_device).

Frames that see a rigid target of known tag poses (a localize.TagMap: a planar board from TagMap.grid or any surveyed 3D
arrangement) give fx, fy, cx, cy, 0 / 4 / 5 distortion coefficients (k1 k2 p1 p2 [k3], the camera model of the PnP),
every frame's camera pose and the standard deviation of each intrinsic (k_calib.inc: closed-form focal lengths -> per-frame
seed -> joint Levenberg-Marquardt with the frames' poses eliminated by the Schur complement).  Calibrate once, then pass
CalibrationResult.camera_params to TagDetector.

A fisheye (lens_model "fisheye": the cv2.fisheye model, 0 or 4 coefficients k1 k2 k3 k4) is calibrated from the corners of
its RAW frames by the same solve under that lens (asl_calibrate_lens_batch; the focal length starts from a ladder of trial
values, since the closed form assumes a pinhole).  Its result goes on as CalibrationResult.view_set(..) -- the rotated
pinhole views every rig solver takes -- or as TagDetector(cr.camera_params, lens_model="fisheye", rectify=True).

    CALIB_RESULT_DTYPE  the asl_calib_result record: K 3x3, dist (5,), std (9,), rms_px, rms_init_px, n_frames_used,
                        n_corners, iterations, status
    CalibrationResult   that record with the per-frame CAM_POSE_DTYPE records, as arrays
"""
import numpy as np

from ._lib import CALIB_RESULT_DTYPE, CAM_POSE_DTYPE

FIX_PRINCIPAL_POINT, FIX_ASPECT_RATIO, ZERO_TANGENT_DIST = 1, 2, 4
STATUS_OK, STATUS_TOO_FEW, STATUS_NO_FOCAL, STATUS_FAILED = 0, 1, 2, 3
STD_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
STD_NAMES_FISHEYE = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "-")

__all__ = ["CALIB_RESULT_DTYPE", "CAM_POSE_DTYPE", "CalibrationResult", "FIX_PRINCIPAL_POINT", "FIX_ASPECT_RATIO",
           "ZERO_TANGENT_DIST", "STATUS_OK", "STATUS_TOO_FEW", "STATUS_NO_FOCAL", "STATUS_FAILED", "STD_NAMES", "STD_NAMES_FISHEYE"]


def rot_to_rvec(R):
    """axis * angle of a rotation matrix (the inverse of tag_detector.rodrigues)"""
    R = np.asarray(R, dtype=np.float64)
    c = np.clip((np.trace(R) - 1) / 2, -1.0, 1.0)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(w)
    theta = np.arctan2(s, c)
    if s > 1e-7:
        return w * (theta / (2 * s))
    if c > 0:
        return 0.5 * w
    vals, vecs = np.linalg.eigh(0.5 * (R + R.T))   # theta ~ pi: the axis is the eigenvector of eigenvalue 1
    return vecs[:, np.argmax(vals)] * theta


class CalibrationResult:
    """K (3x3), dist (n_dist,), std (9,: fx fy cx cy k1 k2 p1 p2 k3, 0 for fixed / unused), rms_px, rms_init_px, status,
    n_frames_used, n_corners, iterations, and poses: (n_frames,) CAM_POSE_DTYPE, world<-camera (status 0: used).
    lens_model "fisheye": dist is k1 k2 k3 k4 and std fx fy cx cy k1 k2 k3 k4 (STD_NAMES_FISHEYE)."""

    def __init__(self, record, poses, n_dist, lens_model="brown"):
        if lens_model not in ("brown", "fisheye"):
            raise ValueError("lens_model must be 'brown' or 'fisheye'")
        r = np.asarray(record, dtype=CALIB_RESULT_DTYPE).reshape(())
        self.record = r.copy()
        self.n_dist = int(n_dist)
        self.lens_model = lens_model
        self.K = np.array(r["K"])
        self.dist = np.array(r["dist"][:self.n_dist])
        self.std = np.array(r["std"])
        self.rms_px = float(r["rms_px"])
        self.rms_init_px = float(r["rms_init_px"])
        self.status = int(r["status"])
        self.n_frames_used = int(r["n_frames_used"])
        self.n_corners = int(r["n_corners"])
        self.iterations = int(r["iterations"])
        self.poses = np.array(poses, dtype=CAM_POSE_DTYPE)

    @property
    def ok(self):
        return self.status == STATUS_OK

    @property
    def camera_params(self):
        """{"camera_matrix": 3x3, "dist_coeffs": (n_dist, 1), "lens_model"}: what TagDetector (and load_camera_calibration)
        take; a fisheye's go to TagDetector(.., lens_model="fisheye", rectify=True)"""
        return {"camera_matrix": self.K.copy(), "dist_coeffs": self.dist.reshape(-1, 1).copy(), "lens_model": self.lens_model}

    def view_set(self, n_views, hfov_deg, size, **kw):
        """rectify.ViewSet.fan of the calibrated camera: n_views pinholes of hfov_deg, size = (w_out, h_out); kw as fan
        takes them (step_deg, axis, theta_max, fill).  Its rig() is what Rig.localize / build_map / locate_tags take."""
        from .rectify import ViewSet
        if not self.ok:
            raise ValueError("calibration failed (status %d): no camera to rectify" % self.status)
        return ViewSet.fan(self.K, self.dist, self.lens_model, n_views, hfov_deg, size, **kw)

    def camera_from_world(self):
        """(rvecs (F, 3, 1), tvecs (F, 3, 1)) camera<-world of the used frames, in frame order"""
        rv, tv = [], []
        for p in self.poses[self.poses["status"] == 0]:
            T = np.linalg.inv(p["T"])
            rv.append(np.asarray(rot_to_rvec(T[:3, :3]), dtype=np.float64).reshape(3, 1))
            tv.append(T[:3, 3].reshape(3, 1))
        return np.array(rv).reshape(-1, 3, 1), np.array(tv).reshape(-1, 3, 1)

    def save_npz(self, path):
        """The calibration file the reference's calibration tool writes (keys camera_matrix, dist_coeffs, rvecs, tvecs);
        video_detection.load_camera_calibration reads it.  A fisheye's file also has the key lens_model, which that loader
        hands on; a Brown file is what it always was."""
        if not self.ok:
            raise ValueError("calibration failed (status %d): nothing to save" % self.status)
        rvecs, tvecs = self.camera_from_world()
        extra = {"lens_model": np.array(self.lens_model)} if self.lens_model != "brown" else {}
        np.savez(path, camera_matrix=self.K, dist_coeffs=self.dist.reshape(-1, 1), rvecs=rvecs, tvecs=tvecs, **extra)

    def __repr__(self):
        return ("CalibrationResult(%sstatus=%d, fx=%.3f, fy=%.3f, cx=%.3f, cy=%.3f, dist=%s, rms_px=%.4f, frames=%d)"
                % ("fisheye, " if self.lens_model == "fisheye" else "", self.status, self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2], np.array2string(self.dist, precision=5),
                   self.rms_px, self.n_frames_used))
