"""Inputs of the tag-location tests (tests/test_locate_ref.py on the CPU, tests/test_gpu_locate.py on the device): asl_obs
blocks of localize_cases' scene (exact projections at 1280x720, TAG_INNER), frame poses and partial maps.

A case is (name, obs (n_frames, max_tags), poses (n_frames,) CAM_POSE_DTYPE, map_in (n_ids,) MAP_TAG_DTYPE, dist, gate,
min_views).  The poses come from localize_ref.localize against the case's partial map, except in frames_edge and
slots_edge, whose blocks hold too few mapped tags (or too many frames) for that: there they are the true camera poses
with the status the case wants.  case(name) builds one case, CASES names them all."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
from aprilslam_amd import _lib, synth
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap

K = synth.camera_matrix(LC.W, LC.H, 45.0)
TAG = LC.TAG_INNER
GATE = 2.0
DIST4 = np.array([-0.08, 0.03, 0.0008, -0.0006])
DIST5 = np.array([-0.12, 0.05, 0.001, -0.0015, 0.01])
SPOILINGS = ("shift", "corner", "neighbour")
SIZED_ID, SIZED_SIDE = 7, 25.0


@functools.lru_cache(maxsize=None)
def scene():
    return LC.bench_scene()


def truth():
    return TagMap.from_scene(scene())


def arc(n):
    """n cameras on the first half of localize_cases.trajectory's loop, as its cpu_cases use"""
    return LC.trajectory(2 * n)[:n]


def partial_map(wanted, n_ids=None):
    """the scene's map with the ids of `wanted` left out (valid = 0, all-zero entries)"""
    rec = truth().as_records()
    if n_ids is not None:
        grown = np.zeros(n_ids, dtype=_lib.MAP_TAG_DTYPE)
        grown[:len(rec)] = rec[:n_ids]
        rec = grown
    for i in wanted:
        rec[i] = np.zeros((), dtype=_lib.MAP_TAG_DTYPE)
    return rec


def odd_ids():
    return [int(t["id"]) for t in scene() if t["id"] % 2 == 1]


def block(cams, dist=None, max_tags=24, tags=None):
    return np.stack([LC.exact_frame(tags if tags is not None else scene(), p, r, K, dist=dist, max_tags=max_tags) for p, r in cams])


def true_poses(cams, status=0):
    out = np.zeros(len(cams), dtype=CAM_POSE_DTYPE)
    for f, (p, r) in enumerate(cams):
        out["T"][f] = LC.world_from_camera(p, r)
    out["status"] = status
    out["seed_slot"] = -1
    return out


def slot_of(obs, f, i):
    hit = np.flatnonzero(((obs["flags"][f] & 1) != 0) & (obs["id"][f] == i))
    assert len(hit), (f, i)
    return int(hit[0])


def remove(obs, f, i):
    """id i out of frame f, if it is there"""
    hit = (obs["id"][f] == i)
    obs["id"][f, hit] = -1
    obs["flags"][f, hit] = 0


def spoil(obs, f, i, how, rng=None):
    """one view's corners spoiled in place: "shift" all corners +6 px, "corner" one corner coordinate +8 px, "neighbour"
    the corners of the next slot, "random" every coordinate by rng's uniform +-12 px"""
    s = slot_of(obs, f, i)
    if how == "shift":
        obs["corners"][f, s] += np.float32(6.0)
    elif how == "corner":
        obs["corners"][f, s, 2] += np.float32(8.0)
    elif how == "neighbour":
        s2 = s + 1 if s + 1 < obs.shape[1] and obs["flags"][f, s + 1] & 1 else s - 1
        obs["corners"][f, s] = obs["corners"][f, s2]
    else:
        obs["corners"][f, s] += rng.uniform(-12.0, 12.0, 8).astype(np.float32)


def sized_view(tag, pos, rot, side, dist=None):
    """(corners (8,) float32, T (12,)) of `tag` seen at its own side, with the PnP pose a solve at TAG gives for it: the true
    camera<-tag with its translation divided by k = h_id / half (sized_cases.block)"""
    T = synth.camera_from_tag(tag["position"], tag["rotation"], pos, rot).copy()
    h = LR.size_half(side, TAG)[0]
    obj = np.array([[-h, -h, 0.0], [h, -h, 0.0], [h, h, 0.0], [-h, h, 0.0]])
    uv = LR.project(LR.camera(K, dist), obj @ T[:3, :3].T + T[:3, 3])
    assert np.all(uv >= 0) and np.all(uv[:, 0] < LC.W) and np.all(uv[:, 1] < LC.H)
    T[:3, 3] /= h / LR.half_size(TAG)
    return uv.ravel().astype(np.float32), T.ravel()[:12]


def located(name, obs, map_in, dist=None, gate=0.0, min_views=2):
    """a case whose poses are localize_ref's against its map"""
    return name, obs, LR.localize(obs, map_in, K, dist, TAG), map_in, dist, gate, min_views


def _views_edge(count, min_views):
    cams = arc(17)
    obs = block(cams)
    for f in range(count, len(cams)):
        remove(obs, f, 1)
    return located("views_edge_%d_min%d" % (count, min_views), obs, partial_map([1]), min_views=min_views)


def _seeds_edge():
    """id 1: 9 seeding views, the two of smallest area tie (the ninth frame repeats the one where the tag is smallest), so
    the top 8 leave out the later of them; id 3: no view with a PnP; id 5: its only PnP is not in its largest view"""
    cams = arc(8)
    first = block(cams)
    areas = [LR.corner_area(first["corners"][f, slot_of(first, f, 1)]) for f in range(8)]
    cams = cams + [cams[int(np.argmin(areas))]]
    obs = block(cams)
    for f in range(len(cams)):
        obs["flags"][f, slot_of(obs, f, 3)] = 1
    a5 = [LR.corner_area(obs["corners"][f, slot_of(obs, f, 5)]) for f in range(len(cams))]
    keep = int(np.argsort(a5)[len(a5) // 2])
    for f in range(len(cams)):
        if f != keep:
            obs["flags"][f, slot_of(obs, f, 5)] = 1
    return located("seeds_edge", obs, partial_map([1, 3, 5]))


def _frames_edge(n):
    """the wanted id 1 seen only in frames 0, 63, 64 and the last (those that exist): the chunk edges of the frame scan.
    Frames of 4 slots: ids 0, 1, 2 and an empty one.  n = 130 also holds views that do not count: frames 10, 11, 12 with
    status 1, 2, 4 and frame 13 with a NaN in its T (all four with spoiled corners, so that using one would show), a second
    slot with the id in frame 0 (spoiled too: the first slot counts); frame 64 has status 6 and counts."""
    cams = arc(n)
    tags = [t for t in scene() if t["id"] in (0, 1, 2)]
    obs = block(cams, max_tags=4, tags=tags)
    poses = true_poses(cams)
    seen = sorted({0, 63, 64, n - 1} & set(range(n)))
    extra = [10, 11, 12, 13] if n == 130 else []
    for f in range(n):
        if f not in seen and f not in extra:
            remove(obs, f, 1)
    if n == 130:
        for f, st in zip(extra, (1, 2, 4, 0)):
            spoil(obs, f, 1, "shift")
            poses["status"][f] = st
        poses["T"][13, 1, 2] = np.nan
        poses["status"][64] = 6
        obs[0, 3] = obs[0, slot_of(obs, 0, 1)]
        obs["corners"][0, 3] += np.float32(9.0)
    return "frames_edge_%d" % n, obs, poses, partial_map([1], n_ids=3), None, 0.0, 2


def _slots_edge(max_tags):
    cams = arc(4)
    poses = true_poses(cams)
    if max_tags == 1:       # one slot a frame, one id in the map
        tags = [t for t in scene() if t["id"] == 0]
        return "slots_edge_1", block(cams, max_tags=1, tags=tags), poses, partial_map([0], n_ids=1), None, 0.0, 2
    # 256 slots a frame, n_ids = 2115 with three ids seen (scene tags 1, 3, 5 as ids 2114, 1000 and 5), ids outside the map
    # and empty slots in between; id 77 is wanted and nobody sees it; id 9 is valid and seen
    relabel = {1: 2114, 3: 1000, 5: 5, 9: 9}
    src = block(cams)
    obs = np.zeros((len(cams), 256), dtype=_lib.OBS_DTYPE)
    obs["id"] = -1
    obs[:, 1::7] = (5000, 3, np.arange(8, dtype=np.float32) * 50, np.eye(4).ravel()[:12])   # ids >= n_ids
    obs[:, 2::7] = (-1, 1, np.arange(8, dtype=np.float32) * 30, np.eye(4).ravel()[:12])     # flags & 1 with id -1
    for f in range(len(cams)):
        for k, (i, new) in enumerate(relabel.items()):
            rec = src[f, slot_of(src, f, i)].copy()
            rec["id"] = new
            obs[f, (0, 100, 255, 4)[k]] = rec
    full = truth().as_records()
    map_in = np.zeros(2115, dtype=_lib.MAP_TAG_DTYPE)
    map_in[9] = full[9]
    map_in[20:40]["valid"] = 1
    map_in["T"][20:40] = np.eye(4).ravel()[:12]
    return "slots_edge_256", obs, poses, map_in, None, 0.0, 2


def _wanted():
    """odd ids left out of the map; id 1 with size -1 and id 3 with size inf are not wanted although seen; id SIZED_ID has
    the side SIZED_SIDE in its entry: its corners are rendered at that side and its PnP pose is the one solved at TAG"""
    cams = arc(8)
    obs = block(cams)
    tag = [t for t in scene() if t["id"] == SIZED_ID][0]
    for f, (p, r) in enumerate(cams):
        s = slot_of(obs, f, SIZED_ID)
        obs["corners"][f, s], obs["T"][f, s] = sized_view(tag, p, r, SIZED_SIDE)
    map_in = partial_map(odd_ids())
    map_in["size"][1], map_in["size"][3], map_in["size"][SIZED_ID] = -1.0, np.inf, SIZED_SIDE
    return located("wanted", obs, map_in)


def gate_frame(i):
    """the frame whose view of odd id i the gate cases spoil"""
    return (i // 2) % 8


def _gate(how, gate):
    obs = block(arc(8))
    for i in odd_ids():
        spoil(obs, gate_frame(i), i, how)
    return located("gate_%s_%s" % (how, "on" if gate else "off"), obs, partial_map(odd_ids()), gate=gate)


def _gate_cap():
    """id 1: 9 of its 17 views spoiled at random, one more than the gate may drop; id 3: two views, one spoiled: the gate
    never drops the last view"""
    cams = arc(17)
    obs = block(cams)
    rng = np.random.default_rng(11)
    for f in range(0, 17, 2):
        spoil(obs, f, 1, "random", rng)
    for f in range(2, 17):
        remove(obs, f, 3)
    spoil(obs, 1, 3, "shift")
    return located("gate_cap", obs, partial_map([1, 3]), gate=GATE)


def _noise():
    obs = block(arc(32))
    rng = np.random.default_rng(7)
    used = (obs["flags"] & 1) != 0
    obs["corners"][used] += rng.normal(0.0, 0.3, obs["corners"][used].shape).astype(np.float32)
    return located("noise", obs, partial_map(odd_ids()))


BUILDERS = {
    "exact": lambda: located("exact", block(arc(8)), partial_map(odd_ids())),
    "mirrored": lambda: located("mirrored", LC.mirror_all(block(arc(8))), partial_map(odd_ids())),
    "views_edge_1_min1": lambda: _views_edge(1, 1),
    "views_edge_1_min2": lambda: _views_edge(1, 2),
    "views_edge_2_min2": lambda: _views_edge(2, 2),
    "views_edge_15_min2": lambda: _views_edge(15, 2),
    "views_edge_16_min2": lambda: _views_edge(16, 2),
    "views_edge_17_min2": lambda: _views_edge(17, 2),
    "seeds_edge": _seeds_edge,
    "frames_edge_63": lambda: _frames_edge(63),
    "frames_edge_64": lambda: _frames_edge(64),
    "frames_edge_65": lambda: _frames_edge(65),
    "frames_edge_130": lambda: _frames_edge(130),
    "slots_edge_1": lambda: _slots_edge(1),
    "slots_edge_256": lambda: _slots_edge(256),
    "wanted": _wanted,
    "gate_cap": _gate_cap,
    "dist4": lambda: located("dist4", block(arc(8)[:4], dist=DIST4), partial_map(odd_ids()), dist=DIST4),
    "dist5": lambda: located("dist5", block(arc(8)[:4], dist=DIST5), partial_map(odd_ids()), dist=DIST5),
    "noise": _noise,
}
for _how in SPOILINGS:
    BUILDERS["gate_%s_on" % _how] = functools.partial(_gate, _how, GATE)
    BUILDERS["gate_%s_off" % _how] = functools.partial(_gate, _how, 0.0)
CASES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c[0] == name
    return c


def pose_errors(T34, T_true):
    """(translation error in scene units, rotation error in rad) of a 3x4 world<-tag against the 4x4 truth"""
    T = np.asarray(T34, dtype=np.float64).reshape(3, 4)
    return float(np.linalg.norm(T[:, 3] - T_true[:3, 3])), LC.rot_err(T, T_true)
