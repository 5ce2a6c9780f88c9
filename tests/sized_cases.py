"""Inputs of the sized-map tests (tests/test_sized_ref.py on the CPU, tests/test_gpu_sized.py on the device): tag maps
whose entries carry their own size, asl_obs blocks from exact projections of those tags at their true sizes, and records
whose PnP pose is what a PnP at the call's single tag_size gives for them: the true camera<-tag with its translation
divided by k = h_id / half (localize_ref.py).  All from 4x4 matrices with localize_ref.project, as rig_cases.py."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import rig_cases as RC
import rig_ref as RR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import TagMap
from aprilslam_amd.rig import Rig, RigCamera

K = synth.camera_matrix(LC.W, LC.H, 45.0)
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
TAG = LC.TAG_INNER                              # 10.0: exact in float32, and so is every ratio below times it
RATIOS = (0.25, 0.5, 1.5, 2.0, 3.0, 4.0)        # a sized tag's side over the call's tag_size
SIGMA = 0.5
# the records' PnP error on the wall.  rig_cases' 0.02 rad about the camera would move a tag 200 units away by 4 units (17
# px), while the mirrored planar minimum of one small tag fits its corners to a pixel or two: a one-tag frame whose PnP pose is
# off by more scores the mirrored candidate better and ends there (measured: a 43 px tag alone, mirrored minimum at 0.57 px
# RMS).  These move a tag by about 0.03 units, a tenth of a pixel: the candidates of a frame still differ far above rounding
PNP_ROT_SIGMA, PNP_TRANS_REL_SIGMA = 0.000125, 0.00006


def one_camera(Kc=K, dist=None):
    return Rig([RigCamera(Kc, dist, np.eye(4))])


def pair():
    """rig_cases' side-by-side pair"""
    return Rig([RigCamera(K, None, RC.mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(K, None, RC.mounting(7.0, (4.0, 0.5, 0.0), 2.0))])


def is_sized(i):
    return i % 3 == 1


@functools.lru_cache(maxsize=None)
def wall(rows=9, cols=9, spacing=11.0, distance=200.0, seed=5):
    """TagMap of rows x cols tags in front of a camera that rests at the world origin looking along +z, each tilted 25 to
    45 degrees (a one-tag frame must tell the tag's two planar minima apart) and set back or forth by up to 15 units (TAG
    is 43 px across there).  Ids with id % 3 == 1 have a size of their own, TAG times RATIOS in turn (id 1: 0.25, 4: 0.5,
    7: 1.5, 10: 2, 13: 3, 16: 4, 19: 0.25, ...; id 64: 2); the others have none.  (The sized tags overlap their neighbours
    on the wall; the corners are projected, not rendered.)"""
    rng = np.random.default_rng(seed)
    tm = TagMap()
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        ax = rng.normal(size=3)
        T = np.eye(4)
        T[:3, :3] = LR.rodrigues(ax / np.linalg.norm(ax) * np.radians(rng.uniform(25, 45))) @ RC.FRONTAL
        T[:3, 3] = [(c - (cols - 1) / 2) * spacing, (r - (rows - 1) / 2) * spacing, distance + rng.uniform(-15, 15)]
        tm[i] = T
    for k, i in enumerate(i for i in range(rows * cols) if is_sized(i)):
        tm.set_size(i, TAG * RATIOS[k % len(RATIOS)])
    return tm


def rig_poses(n, seed=9, rot=0.01, trans=3.0):
    """world<-rig of n frames about the rest pose"""
    rng = np.random.default_rng(seed)
    return [RC.transform(rng.normal(size=3) * rot, rng.normal(size=3) * trans) for _ in range(n)]


def block(tm, rig, poses, tag_size, max_tags, slot_ids=None, pnp_seed=1, image_sizes=None, pnp_sigmas=(PNP_ROT_SIGMA, PNP_TRANS_REL_SIGMA)):
    """(n_cams, n_frames, max_tags) asl_obs, camera-major, of the map tm (a TagMap with sizes) seen by rig at poses
    (world<-rig per frame).  slot_ids None: every tag in view of camera c in frame f, in id order (rig_cases.exact_block).
    Otherwise slot_ids[c][f] is the list of ids for the slots of that camera and frame in slot order (-1: an empty slot),
    every one of which must be in view.  Corners: the tag's true corners, at its own half, projected exactly and rounded to
    float32.  T: the true camera<-tag, moved by a small seeded PnP error as in rig_cases (pnp_sigmas;
    pnp_seed None: not moved), then its translation divided by k = h_id / half for a sized tag: what a PnP at tag_size gives."""
    rec = tm.as_records()
    rng = np.random.default_rng(pnp_seed)
    obs = np.zeros((len(rig), len(poses), max_tags), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    half = LR.half_size(tag_size)
    for c, rc in enumerate(rig.cameras):
        cam = LR.camera(rc.K, rc.dist)
        w, h = image_sizes[c] if image_sizes else (LC.W, LC.H)
        for f, Twr in enumerate(poses):
            Tcw = rc.T_cam_rig @ np.linalg.inv(Twr)
            ids = tm.ids() if slot_ids is None else slot_ids[c][f]
            k = 0
            for i in ids:
                if i < 0:
                    k += 1
                    continue
                hid, own = LR.tag_half(rec[i], tag_size)
                obj = np.c_[LR.half_corners(hid), np.zeros(4)]
                T = Tcw @ tm[i]
                P = obj @ T[:3, :3].T + T[:3, 3]
                uv = LR.project(cam, P) if np.all(P[:, 2] > 1e-3) else np.full((4, 2), -1.0)
                seen = not (np.any(uv < 0) or np.any(uv[:, 0] >= w) or np.any(uv[:, 1] >= h))
                if slot_ids is not None:
                    assert seen and k < max_tags, (c, f, i)
                elif not seen or k >= max_tags:
                    continue
                if pnp_seed is not None:
                    T = RC.transform(rng.normal(size=3) * pnp_sigmas[0], rng.normal(size=3) * pnp_sigmas[1] * np.linalg.norm(T[:3, 3])) @ T
                if own:
                    T = T.copy()
                    T[:3, 3] = T[:3, 3] / (hid / half)
                obs[c, f, k] = (i, 3, uv.ravel(), T.ravel()[:12])
                k += 1
    return obs


def mirror_slot(obs, f, s):
    """slot s of frame f: its PnP pose replaced by its mirrored planar minimum (obs (n_frames, max_tags), in place)"""
    T = obs["T"][f, s].reshape(3, 4)
    R, t = LR.mirrored(T[:, :3], T[:, 3])
    obs["T"][f, s] = np.c_[R, t].ravel()


def without_sizes(rec):
    out = rec.copy()
    out["size"] = 0
    return out


# ---- the truth: a small mixed-size scene with exact corners and exact records

def small_map(sized=True):
    """6 tags about 120 units in front of the rest pose (72 px across at TAG), id 5 of side 2 TAG if sized"""
    rng = np.random.default_rng(3)
    tm = TagMap()
    for i in range(6):
        ax = rng.normal(size=3)
        T = np.eye(4)
        T[:3, :3] = LR.rodrigues(ax / np.linalg.norm(ax) * np.radians(rng.uniform(20, 40))) @ RC.FRONTAL
        T[:3, 3] = [(i % 3 - 1) * 40.0, (i // 3 - 0.5) * 50.0, 120.0 * rng.uniform(0.9, 1.1)]
        tm[i] = T
    if sized:
        tm.set_size(5, 2 * TAG)
    return tm


def truth_case(sized=True):
    """(obs (6, 4), map records, truths (6 world<-camera)): 6 frames, max_tags 4, n_ids 6; every frame sees three of the
    tags 0..4 and tag 5, exact corners, every record's T the true pose (translation / k for tag 5)"""
    tm = small_map(sized)
    poses = rig_poses(6, seed=4, rot=0.03, trans=2.0)
    ids = [[sorted((f + j) % 5 for j in range(3)) + [5] for f in range(6)]]
    return block(tm, one_camera(), poses, TAG, 4, slot_ids=ids, pnp_seed=None)[0], tm.as_records(), poses


def truth_err(poses, truths):
    return max(LC.rel_err(p["T"], t) for p, t in zip(poses, truths))


@functools.lru_cache(maxsize=None)
def truth_bar():
    """(the statement's error against the truth on the equal-size scene of truth_case's geometry, the bar: ten times it for
    the different rounding path of a sized map).  Measured with the statement on the CPU, never with the kernels."""
    obs, rec, truths = truth_case(sized=False)
    base = truth_err(LR.localize(obs, rec, K, None, TAG), truths)
    return base, 10 * base


def uniform_case(s1, s2):
    """one physical scene of tags of side s2, described twice: (obs_a, rec_a): every entry sized s2, the call at s1, records
    solved at s1; (obs_b, rec_b): sizes 0, the call at s2, records solved at s2.  The corners are the same bytes.  The
    records' PnP error is rig_cases' own: the tags are at its 120 units."""
    tm = small_map(False)
    poses = rig_poses(6, seed=4, rot=0.03, trans=2.0)
    ids = [[sorted((f + j) % 6 for j in range(4)) for f in range(6)]]
    sized = TagMap(tm.poses, {i: s2 for i in tm.ids()})
    far = (RC.PNP_ROT_SIGMA, RC.PNP_TRANS_REL_SIGMA)
    a = block(sized, one_camera(), poses, s1, 4, slot_ids=ids, pnp_sigmas=far)[0]
    b = block(tm, one_camera(), poses, s2, 4, slot_ids=ids, pnp_sigmas=far)[0]
    assert a["corners"].tobytes() == b["corners"].tobytes()
    return (a, sized.as_records()), (b, tm.as_records())


# ---- kernel against statement

LOC_MAX_TAGS = (1, 2, 64, 65)
GATE = 2.0


@functools.lru_cache(maxsize=None)
def loc_case(max_tags, dist5=False):
    """(obs (8, max_tags), map records, dist, notes) on the wall.  The gate of the call is GATE; only frame 3 has a slot over it.
      0  slots 0.. hold ids 0.., all seeding: mixed, slot 64 (id 64) a sized one at max_tags 65
      1  as 0, only the sized slots seed: the winning seed is a sized slot (max_tags 1: id 10 alone)
      2  as 1, the sized slots' PnP poses mirrored: the winner is the mirrored candidate of a sized slot
      3  as 0 with one corner of one sized slot moved by 12 px in x and y (a whole tag moved could be followed by the pose
         of a frame of two): the gate drops it (max_tags >= 2)
      4  only a sized tag (id 16), in the last slot
      5  only a tag without a size (id 0)
      6  as 0 with every fifth slot empty and slot 0 an id outside the map
      7  sized tags only (ids 10, 13, 16, 7, 4, 1, 19, 22, ...: the larger ones first, a tag of 5 px alone holds no pose)
    notes: {frame: the sized slots the frame is about}"""
    tm = wall()
    dist = DIST5 if dist5 else None
    mt = max_tags
    base = list(range(mt)) if mt > 1 else [10]
    f6 = [-1 if s % 5 == 4 else i for s, i in enumerate(base)]
    ids = [base, base, base, base, [-1] * (mt - 1) + [16], [0] + [-1] * (mt - 1), f6, ([10, 13, 16, 7, 4, 1] + [3 * s + 1 for s in range(6, 27)])[:mt]]
    obs = block(tm, one_camera(K, dist), rig_poses(8), TAG, mt, slot_ids=[ids])[0]
    sized = [s for s, i in enumerate(base) if is_sized(i)]
    for f in (1, 2):
        for s in range(mt):
            if s not in sized:
                obs["flags"][f, s] &= 1
    for s in sized:
        mirror_slot(obs, 2, s)
    notes = {1: sized, 2: sized, 4: [mt - 1]}
    if mt >= 2:
        obs["corners"][3, sized[-1], :2] += 12.0
        notes[3] = [sized[-1]]
    obs["id"][6, 0] = 999
    return obs, tm.as_records(), dist, notes


@functools.lru_cache(maxsize=None)
def rig_case():
    """(obs (2, 6, 3), map records, rig): frames 0, 1: both cameras see sized and unsized tags; 2, 3: the sized tag only in
    camera 1; 4: camera 0 sees nothing, camera 1 a sized tag alone; 5: sized tags only"""
    tm, rig = wall(), pair()
    ids = [[[30, 31, 32], [39, 40, 41], [30, 32, 33], [38, 39, 41], [-1, -1, -1], [31, 34, 37]],
           [[48, 49, 50], [40, 42, 44], [47, 49, 50], [46, 48, 50], [-1, 43, -1], [40, 43, 46]]]
    return block(tm, rig, rig_poses(6, seed=2), TAG, 3, slot_ids=ids), tm.as_records(), rig


def noisy(obs, px, seed):
    out = obs.copy()
    rng = np.random.default_rng(seed)
    out["corners"] = (out["corners"].astype(np.float64) + rng.normal(0.0, px, out["corners"].shape)).astype(np.float32)
    return out


SMOOTH_SIGMAS = (0.5, 0.01, 0.2)     # smooth_cases.SHAPE_SIGMAS
SMOOTH_ITERS = 3                     # smooth_cases.COMPARE_ITERS: the trials of the steep part, where the comparison is of the arithmetic
SMOOTH_POSES = dict(rot=0.004, trans=0.6)


def walk(n, seed):
    """world<-camera of n consecutive frames: a random walk of small steps from the rest pose"""
    rng = np.random.default_rng(seed)
    out, T = [], np.eye(4)
    for _ in range(n):
        T = T @ RC.transform(rng.normal(size=3) * SMOOTH_POSES["rot"], rng.normal(size=3) * SMOOTH_POSES["trans"])
        out.append(T)
    return out


@functools.lru_cache(maxsize=None)
def smooth_case():
    """(obs (12, 3), map records, seeds): smooth_cases.shape's recipe on the wall: corners with 0.2 px noise, seeded by the
    (sized) localisation of the same frames without it.  Frames 2 and 6 see nothing; frames 3, 4 and 7 see one sized tag alone
    (candidate B), the seed of frame 4 replaced by its mirrored minimum"""
    import smooth_cases as SC
    import smooth_ref as SR
    tm = wall()
    ids = [[[39, 40, 41], [40, 42, 44], [-1, -1, -1], [-1, 37, -1], [37, -1, -1], [38, 39, 43], [-1, -1, -1], [-1, -1, 49], [30, 31, 32],
            [46, 47, 48], [40, -1, 41], [31, 34, 41]]]
    exact = block(tm, one_camera(), walk(12, 6), TAG, 3, slot_ids=ids)[0]
    rec = tm.as_records()
    obs = noisy(exact, 0.2, 1203)
    seed = LR.localize(exact, rec, K, None, TAG)
    seed = SC.mirror_seed(SR.problem(obs, rec, K, None, TAG, *SMOOTH_SIGMAS), seed, (4,))
    return obs, rec, seed


@functools.lru_cache(maxsize=None)
def smooth_rig_case():
    """(obs (2, 8, 3), map records, rig, seeds): the same recipe for the pair; frame 3 sees nothing, frame 5 one sized tag in
    camera 1 alone"""
    tm, rig = wall(), pair()
    ids = [[[30, 31, 32], [39, 40, 41], [30, 32, 33], [-1, -1, -1], [38, 39, 41], [-1, -1, -1], [31, 34, 37], [40, -1, 41]],
           [[48, 49, 50], [40, 42, 44], [47, 49, 50], [-1, -1, -1], [46, -1, 50], [-1, 43, -1], [40, 43, 46], [-1, -1, -1]]]
    exact = block(tm, rig, walk(8, 8), TAG, 3, slot_ids=ids)
    rec = tm.as_records()
    return noisy(exact, 0.2, 803), rec, rig, RR.localize(exact, rec, rig, TAG)


CALIB_FRAMES = 6      # the fewest frames of a board in calib_cases.cpu_cases (the fronto-parallel board)


@functools.lru_cache(maxsize=None)
def calib_case(n_dist):
    """(obs (6, 40), map records): calib_cases' tilted board views through K_TRUE and n_dist coefficients, the board's odd ids of
    side 14 (spacing 16), the even ones without a size (TAG)"""
    import calib_cases as CC
    tm = TagMap.grid(CC.BOARD_ROWS, CC.BOARD_COLS, TAG, CC.BOARD_SPACING)
    for i in tm.ids():
        if i % 2:
            tm.set_size(i, 14.0)
    poses = [LC.world_from_camera(p, r) for p, r in CC.board_cameras(CALIB_FRAMES)]
    dist = CC.DIST5 if n_dist else None
    return block(tm, one_camera(CC.K_TRUE, dist), poses, TAG, 40)[0], tm.as_records()
