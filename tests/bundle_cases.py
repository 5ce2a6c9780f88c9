"""Inputs of the tag-bundle tests (tests/test_bundle_ref.py on the CPU, tests/test_gpu_bundles.py on the device): three
bundles that move independently in front of a moving camera, as asl_obs blocks of exact projections, with the ground truth.

Every number is the smallest at which the indexing of the bundle dimension can go wrong:
  bundles     0: one tag (id 5, of its own size 20); 1: two tags (ids 2 and 9, id 9 of its own size 6); 2: four tags (ids 0, 3,
              6, 11); id 7 is seen in every frame and is in no bundle.  The ids interleave, so a frame's slots in id order
              (0 2 3 5 6 7 9 11) alternate between the bundles.  n_ids = 12.
  frames      5.  In frame 1 bundle 1 is out of view (its records are not there: status 1); in frame 3 the only tag of
              bundle 0 has flags & 2 cleared (corners but no PnP pose: status 2).  Every other (frame, bundle) is meant to be posed.
  max_tags    4 (the first four slots of the frame: every bundle still has a tag), 16 (64 corners exactly fill the wave) and
              17 (68 wrap it)
  rig         2 cameras x max_tags 4: bundle 0 is seen by camera 0 only, bundle 1 by both, bundle 2 by camera 1 only
All poses are built from 4x4 matrices and projected with localize_ref.project, like rig_cases."""
import numpy as np

import localize_cases as LC
import localize_ref as LR
import rig_cases as RC
from aprilslam_amd import _lib
from aprilslam_amd.bundles import BundleSet
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

K = RC.K45
TAG_SIZE = 10.0
N_FRAMES, N_IDS = 5, 12
MAX_TAGS = (4, 16, 17)
STRAY_ID = 7
GROUPS = [[5], [2, 9], [0, 3, 6, 11]]
SIZES = {5: 20.0, 9: 6.0}
OUT_OF_VIEW = (1, 1)          # (frame, bundle): no record of the bundle in the frame -> status 1
NO_PNP = (3, 0)               # (frame, bundle): the bundle's only tag has corners but no pose -> status 2
RIG_YAW = 50.0                # camera 1 of the rig looks that far to the side of camera 0
PNP_ROT_SIGMA, PNP_TRANS_REL_SIGMA = 0.002, 0.0005  # the records' PnP poses: off the truth (no two candidates the same pose), and
                                                    # near enough for a bundle of one tag to be seeded in its true minimum


def layouts():
    """[TagMap] of the three bundles, bundle<-tag: no tag at the identity, none coplanar with its neighbours"""
    b0 = TagMap({5: RC.transform((0.05, -0.1, 0.2), (1.0, -2.0, 0.5))}, {5: SIZES[5]})
    b1 = TagMap({2: RC.transform((0.2, 0.1, 0.0), (-9.0, 0.0, 0.0)), 9: RC.transform((-0.15, 0.25, 0.1), (9.0, 1.0, 2.0))}, {9: SIZES[9]})
    b2 = TagMap({i: RC.transform((0.1 * (k - 1.5), 0.12 * (1.5 - k), 0.05 * k), (6.0 * (2 * (k % 2) - 1), 6.0 * (2 * (k // 2) - 1), 1.0 * k))
                 for k, i in enumerate(GROUPS[2])})
    return [b0, b1, b2]


def bundle_set():
    return BundleSet(layouts(), ["tool", "pallet", "pad"])


def tables():
    """(3, N_IDS) MAP_TAG_DTYPE"""
    return bundle_set().table(N_IDS)


def _seen_from(yaw_deg, pitch_deg, offset, distance, tilt):
    """body<-object of an object that a virtual camera at the body's origin, turned by yaw and pitch, sees at `offset` from
    its axis at `distance`, tilted by the rotation vector `tilt` from head-on"""
    T = np.eye(4)
    T[:3, :3] = LR.rodrigues(np.asarray(tilt, dtype=np.float64)) @ RC.FRONTAL
    T[:3, 3] = [offset[0], offset[1], distance]
    return np.linalg.inv(RC.mounting(yaw_deg, pitch_deg=pitch_deg)) @ T


def object_poses(rig=False):
    """(camera<-object [f][k] for the three bundles and, k = 3, the stray tag): independent trajectories, the camera's own
    motion on top.  rig: body = the rig, the objects spread over the two cameras' views."""
    out = []
    for f in range(N_FRAMES):
        s = f - 2.0
        cam = RC.transform((0.01 * s, -0.015 * s, 0.02 * s), (0.4 * s, -0.25 * s, 0.7 * s))      # the camera moves
        if rig:
            place = [(-15.0, 0.0, (1.0 * s, 1.5, 0.0), 65.0), (RIG_YAW / 2, 0.0, (0.0, 5.0 - 1.0 * s, 0.0), 75.0 + 1.5 * s),
                     (RIG_YAW, 0.0, (1.5 * s, -2.5, 0.0), 60.0 - 1.0 * s), (0.0, 14.0, (0.0, 0.0, 0.0), 70.0)]
        else:
            place = [(0.0, 0.0, (-22.5 + 1.0 * s, -7.5, 0.0), 65.0 + 1.0 * s), (0.0, 0.0, (1.5 * s, 11.0, 0.0), 75.0 - 2.0 * s),
                     (0.0, 0.0, (22.5, -5.0 + 1.2 * s, 0.0), 60.0 + 1.5 * s), (0.0, 0.0, (-1.0 * s, -19.0, 0.0), 70.0)]
        tilts = [(0.45 + 0.03 * s, -0.3, 0.1 * s), (-0.35, 0.4 - 0.04 * s, -0.08 * s), (0.3, 0.35 + 0.02 * s, 0.15 * s), (0.2, -0.2, 0.0)]
        out.append([cam @ _seen_from(y, p, o, d, t) for (y, p, o, d), t in zip(place, tilts)])
    return out


def truth(rig=False):
    """(N_FRAMES, 3, 4, 4): the true bundle<-camera (bundle<-rig)"""
    return np.array([[np.linalg.inv(T) for T in row[:3]] for row in object_poses(rig)])


def scene(frame=0):
    """TagMap of every tag in the camera frame of one instant (world = that camera): what a map built with all objects at
    rest holds, for BundleSet.from_map; the stray tag included"""
    row = object_poses()[frame]
    tm = TagMap()
    for b, lay in enumerate(layouts()):
        for i in lay.ids():
            tm[i] = row[b] @ lay[i]
            tm.set_size(i, lay.size(i))
    tm[STRAY_ID] = row[3]
    return tm


def _records(cameras, max_tags, rig, pnp_seed=1):
    """(n_cams, N_FRAMES, max_tags) asl_obs of what each camera (K, dist, camera<-body) sees, slots in id order"""
    lays = layouts()
    rng = np.random.default_rng(pnp_seed)
    obs = np.zeros((len(cameras), N_FRAMES, max_tags), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    half = LR.half_size(TAG_SIZE)
    for f, row in enumerate(object_poses(rig)):
        tags = {STRAY_ID: (row[3], half, False)}
        for b, lay in enumerate(lays):
            if (f, b) == OUT_OF_VIEW:
                continue
            for i in lay.ids():
                h, own = LR.size_half(lay.size(i), TAG_SIZE)
                tags[i] = (row[b] @ lay[i], h, own)
        for c, (Kc, dist, E) in enumerate(cameras):
            cam = LR.camera(Kc, dist)
            k = 0
            for i in sorted(tags):
                Tbt, h, own = tags[i]
                T = E @ Tbt
                P = np.c_[LR.half_corners(h), np.zeros(4)] @ T[:3, :3].T + T[:3, 3]
                if np.any(P[:, 2] <= 1e-3):
                    continue
                uv = LR.project(cam, P)
                if np.any(uv < 0) or np.any(uv[:, 0] >= LC.W) or np.any(uv[:, 1] >= LC.H):
                    continue
                # the record's pose: a single view's PnP error on the truth (rig_cases.exact_block), then, for a tag with a
                # size of its own, as the PnP at the call's tag_size finds it: the translation times half / h
                T = RC.transform(rng.normal(size=3) * PNP_ROT_SIGMA, rng.normal(size=3) * PNP_TRANS_REL_SIGMA * np.linalg.norm(T[:3, 3])) @ T
                if own:
                    T[:3, 3] *= half / h
                if k < max_tags:
                    obs[c, f, k] = (i, 1 if (f, 0) == NO_PNP and i == GROUPS[0][0] else 3, uv.ravel(), T.ravel()[:12])
                k += 1
    return obs


def camera_block(max_tags):
    """(N_FRAMES, max_tags) asl_obs of the one camera"""
    return _records([(K, None, np.eye(4))], max_tags, rig=False)[0]


def rig_of_two():
    return Rig([RigCamera(K, None, np.eye(4)), RigCamera(K, None, RC.mounting(RIG_YAW, (3.0, 0.25, 0.0)))])


def rig_block(max_tags=4):
    """(2, N_FRAMES, max_tags) asl_obs, camera-major, of rig_of_two()"""
    r = rig_of_two()
    return _records([(c.K, None, c.T_cam_rig) for c in r.cameras], max_tags, rig=True)


def noisy(obs, sigma=0.2, seed=12):
    """the block with Gaussian corner noise of sigma pixels"""
    out = obs.copy()
    rng = np.random.default_rng(seed)
    out["corners"] = (out["corners"].astype(np.float64) + rng.normal(scale=sigma, size=out["corners"].shape)).astype(np.float32)
    return out


def meant_posed():
    """(N_FRAMES, 3) bool: the (frame, bundle) pairs meant to be posed"""
    m = np.ones((N_FRAMES, 3), dtype=bool)
    m[OUT_OF_VIEW] = False
    m[NO_PNP] = False
    return m


def expected_status():
    s = np.zeros((N_FRAMES, 3), dtype=np.int32)
    s[OUT_OF_VIEW] = 1
    s[NO_PNP] = 2
    return s


# ---- the statement's results on these inputs, computed once and shared by the tests (do not write into them)

SIGMA = 0.5
_cache = {}


def statement(kind, max_tags=16, sigma_px=SIGMA, noise=False, gate=0.0):
    """(obs, poses (N_FRAMES, 3) CAM_POSE_DTYPE, cov (N_FRAMES, 3) POSE_COV_DTYPE) of bundle_ref on the camera block
    (kind "camera") or the rig block (kind "rig"), cached"""
    import bundle_ref as BR
    key = (kind, max_tags, sigma_px, noise, gate)
    if key not in _cache:
        obs = camera_block(max_tags) if kind == "camera" else rig_block(max_tags)
        if noise:
            obs = noisy(obs)
        if kind == "camera":
            p, c = BR.localize_bundles(obs, tables(), K, None, TAG_SIZE, gate, sigma_px)
        else:
            p, c = BR.localize_bundles_rig(obs, tables(), rig_of_two(), TAG_SIZE, gate, sigma_px)
        _cache[key] = (obs, p, c)
    return _cache[key]


def relative_inputs():
    """[(name, poses, cov)] that the relative-pose checks run over: every max_tags of the camera, and the rig"""
    return [("camera%d" % mt,) + statement("camera", mt)[1:] for mt in MAX_TAGS] + [("rig",) + statement("rig", 4)[1:]]


def cov_reorder_error():
    """e = max_ij |C64 - C_ld|_ij / sqrt(C_ii C_jj) over every posed pair of relative_inputs() and both references: what
    evaluating the relative covariance in float64 instead of np.longdouble costs"""
    import bundle_ref as BR
    e = 0.0
    for _, p, c in relative_inputs():
        for ref in (0, p.shape[1] - 1):
            for f in range(p.shape[0]):
                for b in range(p.shape[1]):
                    if b == ref or p["status"][f, b] or p["status"][f, ref] or c["status"][f, b] or c["status"][f, ref]:
                        continue
                    C64 = BR.relative(p["T"][f, ref], c["cov"][f, ref], p["T"][f, b], c["cov"][f, b])[1]
                    Cld = BR.relative(p["T"][f, ref], c["cov"][f, ref], p["T"][f, b], c["cov"][f, b], np.longdouble)[1]
                    s = np.sqrt(np.diag(Cld).astype(np.float64))
                    e = max(e, float((np.abs(C64 - Cld).astype(np.float64) / np.outer(s, s)).max()))
    return e


def device_cov_bar():
    """The device bar for the relative covariance, in the normalisation of cov_reorder_error: ten times what float64
    reordering alone can cost, and no less than 1e-12 (as test_smooth_ref.py derives its bar)"""
    return max(10.0 * cov_reorder_error(), 1e-12)
