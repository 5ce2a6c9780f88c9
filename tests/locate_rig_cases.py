"""Inputs of the rig tag-location tests (tests/test_locate_rig_ref.py on the CPU, tests/test_gpu_locate_rig.py on the
device): camera-major asl_obs blocks (n_cams, n_frames, max_tags) of rig_cases' rigs (exact projections), world<-rig poses
and partial maps, each at the smallest shape at which its part of asl_locate_tags_rig_* can go wrong.

A case is a dict: name, obs, poses (n_frames,) CAM_POSE_DTYPE, map_in (n_ids,) MAP_TAG_DTYPE, rig, gate, min_views, truth
({wanted id: 4x4 world<-tag}), and what its builder wants checked (views: {id: the (frame, camera) list}, spoiled:
{id: (frame, camera)}, left_out: {id: the list position the top 8 leave out}).  The poses are rig_ref.localize's against
the case's partial map, except in frames_edge and slots_edge, which have too few mapped tags (or too many frames) for
that: there they are the true rig poses with the status the case wants.  The cases that check recovery of the truth carry
the true PnP poses (pnp_seed=None).  case(name) builds one case, CASES names them all."""
import functools

import numpy as np

import localize_cases as LC
import localize_ref as LR
import locate_cases as QC
import rig_cases as RC
import rig_ref as RR
from aprilslam_amd import _lib
from aprilslam_amd.localize import CAM_POSE_DTYPE, TagMap
from aprilslam_amd.rig import Rig, RigCamera

TAG = LC.TAG_INNER
GATE = QC.GATE
SIZED_ID, SIZED_SIDE = QC.SIZED_ID, QC.SIZED_SIDE
MIXED_SIZES = [(LC.W, LC.H), (640, 480)]


def pair():
    """rig_cases' side_by_side rig"""
    return Rig([RigCamera(RC.K45, None, RC.mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(RC.K45, None, RC.mounting(7.0, (4.0, 0.5, 0.0), 2.0))])


def mixed():
    """rig_cases' mixed_models rig: a 1280x720 pinhole camera and a 640x480 camera with 5 lens coefficients"""
    return Rig([RigCamera(RC.K45, None, RC.mounting(-6.0, (-4.0, 0.0, 0.0))), RigCamera(RC.K60, RC.DIST5, RC.mounting(5.0, (4.0, 0.5, 0.0)))])


def ring(n):
    """n cameras fanned out over 28 degrees and 14 units (n = 8: rig_cases' slots_256 rig)"""
    return Rig([RigCamera(RC.K45, None, RC.mounting(-14.0 + 32.0 / n * c, (-7.0 + 16.0 / n * c, 0.3 * (c % 3), 0.0), 1.0 * (c % 2))) for c in range(n)])


def scene_map(ids=None):
    tm = TagMap.from_scene(QC.scene())
    if ids is None:
        return tm
    out = TagMap()
    for i in ids:
        out[i] = tm[i]
    return out


def true_poses(Twr, status=0):
    out = np.zeros(len(Twr), dtype=CAM_POSE_DTYPE)
    out["T"] = np.array(Twr).reshape(-1, 4, 4)
    out["status"] = status
    out["seed_slot"] = -1
    return out


def views_of(obs, i, frames=None):
    """the (frame, camera) of every view of id i in the block, in list order"""
    return [(f, c) for f in (range(obs.shape[1]) if frames is None else frames) for c in range(obs.shape[0])
            if (((obs["flags"][c, f] & 1) != 0) & (obs["id"][c, f] == i)).any()]


def make(name, obs, poses, map_in, rig, truth_map, gate=0.0, min_views=2, **more):
    wanted = [i for i in range(len(map_in)) if not map_in["valid"][i] and i in truth_map.ids()]
    return dict(name=name, obs=obs, poses=poses, map_in=map_in, rig=rig, gate=gate, min_views=min_views,
                truth={i: truth_map[i] for i in wanted}, **more)


def located(name, obs, map_in, rig, truth_map, **kw):
    """a case whose poses are rig_ref's against its map"""
    return make(name, obs, RR.localize(obs, map_in, rig, TAG), map_in, rig, truth_map, **kw)


def _rear_only():
    """the map holds camera 0's tags; ids 2 and 3 are seen by camera 1 alone, which never sees a mapped tag"""
    tm, rig, Twr = RC.back_to_back()
    obs = RC.exact_block(tm, rig, Twr, TAG, 4, pnp_seed=None)
    map_in = tm.as_records()
    map_in[2:4] = np.zeros((), dtype=_lib.MAP_TAG_DTYPE)
    assert all(c == 1 for i in (2, 3) for _, c in views_of(obs, i)) and all(c == 0 for i in (0, 1) for _, c in views_of(obs, i))
    return located("rear_only", obs, map_in, rig, tm)


def _side(name, pnp_seed, n=6, **kw):
    tm = scene_map()
    obs = RC.exact_block(tm, pair(), RC.bench_poses(n), TAG, 24, pnp_seed=pnp_seed)
    return located(name, obs, QC.partial_map(QC.odd_ids()), pair(), tm, **kw)


def _both_cameras():
    c = _side("both_cameras", None)
    c["views"] = {i: views_of(c["obs"], i) for i in QC.odd_ids()}
    assert any(len(v) > len({f for f, _ in v}) for v in c["views"].values())       # a tag with two views in one frame
    return c


def _mixed_models():
    """odd ids wanted; id TOP8_ID has 9 seeding views, 7 in the long-focus camera 0 and the two of smallest area in camera 1,
    which tie (frame 6 repeats the frame where the tag is smallest there): the top 8 leave out the later of the two"""
    tm, rig = scene_map(), mixed()
    Twr = RC.bench_poses(6)
    first = RC.exact_block(tm, rig, Twr, TAG, 24, sizes=MIXED_SIZES, pnp_seed=None)
    i = TOP8_ID
    a1 = {f: LR.corner_area(first["corners"][1, f, QC.slot_of(first[1], f, i)]) for f, c in views_of(first, i) if c == 1}
    k = min(a1, key=a1.get)
    Twr = Twr + [Twr[k]]
    obs = RC.exact_block(tm, rig, Twr, TAG, 24, sizes=MIXED_SIZES, pnp_seed=None)
    views = views_of(obs, i)
    area = [LR.corner_area(obs["corners"][c, f, QC.slot_of(obs[c], f, i)]) for f, c in views]
    assert [v for v in views if v[1] == 0] == [(f, 0) for f in range(7)] and area[views.index((k, 1))] == area[views.index((6, 1))] == min(area)
    for f, c in views:
        if c == 1 and f not in (k, 6):
            obs["flags"][c, f, QC.slot_of(obs[c], f, i)] = 1
    return located("mixed_models", obs, QC.partial_map(QC.odd_ids()), rig, tm, views={i: views}, left_out={i: views.index((6, 1))})


TOP8_ID = 9


def _frames_edge(n):
    """2 cameras, the wanted id 1 in frames 0, 63, 64 and the last (those that exist): in frame 63 and in the last one camera 1
    alone sees it, in the others both cameras do, so the lanes of the frame scan hold 0, 1 and 2 views across its 64-frame
    chunk edges.  Frames of 4 slots: ids 0, 1, 2 and an empty one.  n = 130 also holds views that do not count: frames 10, 11, 12
    with status 1, 2, 4 and frame 13 with a NaN in its T (all with spoiled corners in both cameras, so that using one would
    show), a second slot with the id in camera 0 of frame 0 (spoiled too: the first slot counts); frame 64 has status 6 and
    counts."""
    rig = pair()
    Twr = [LC.world_from_camera(p, r) for p, r in QC.arc(n)]
    obs = RC.exact_block(scene_map((0, 1, 2)), rig, Twr, TAG, 4, pnp_seed=None)
    poses = true_poses(Twr)
    seen = sorted({0, 63, 64, n - 1} & set(range(n)))
    extra = [10, 11, 12, 13] if n == 130 else []
    alone = {63, n - 1}
    for f in seen + extra:
        assert views_of(obs, 1, [f]) == [(f, 0), (f, 1)], f
    for f in range(n):
        for c in range(2):
            if (f not in seen and f not in extra) or (f in seen and f in alone and c == 0):
                QC.remove(obs[c], f, 1)
    if n == 130:
        for f, st in zip(extra, (1, 2, 4, 0)):
            for c in range(2):
                QC.spoil(obs[c], f, 1, "shift")
            poses["status"][f] = st
        poses["T"][13, 1, 2] = np.nan
        poses["status"][64] = 6
        obs[0, 0, 3] = obs[0, 0, QC.slot_of(obs[0], 0, 1)]
        obs["corners"][0, 0, 3] += np.float32(9.0)
    views = [(f, c) for f in seen for c in range(2) if f not in alone or c == 1]
    return make("frames_edge_%d" % n, obs, poses, QC.partial_map([1], n_ids=3), rig, scene_map(), views={1: views})


def _views_edge(count, name=None):
    """id 1: the first `count` of the 18 views 9 frames x 2 cameras give; 15, 16 and 17 are the lane-count edge of the
    corner loop, 2 is min_views = 2 met by one frame's two cameras"""
    tm = scene_map()
    obs = RC.exact_block(tm, pair(), RC.bench_poses(9), TAG, 24, pnp_seed=None)
    views = views_of(obs, 1)
    assert len(views) == 18
    for f, c in views[count:]:
        QC.remove(obs[c], f, 1)
    return located(name or "views_edge_%d" % count, obs, QC.partial_map([1]), pair(), tm, views={1: views[:count]})


def _slots_edge(n_cams, max_tags):
    """n_cams * max_tags = 256 global slots, odd ids wanted, 4 frames"""
    tm, rig = scene_map(), ring(n_cams)
    Twr = RC.bench_poses(4)
    obs = RC.exact_block(tm, rig, Twr, TAG, max_tags, pnp_seed=None)
    return make("slots_edge_%dx%d" % (n_cams, max_tags), obs, true_poses(Twr), QC.partial_map(QC.odd_ids()), rig, tm)


def _slots_edge_1():
    """one camera, one slot a frame, one id in the map"""
    rig = Rig([RigCamera(RC.K45, None, np.eye(4))])
    Twr = RC.bench_poses(4)
    obs = RC.exact_block(scene_map((0,)), rig, Twr, TAG, 1, pnp_seed=None)
    return make("slots_edge_1x1", obs, true_poses(Twr), QC.partial_map([0], n_ids=1), rig, scene_map())


def gate_frame(i):
    """the frame whose camera-1 view of odd id i the gate cases spoil"""
    return (i // 2) % 6


def _gate_per_view(how, gate):
    """camera 1's view of one frame spoiled for every odd id both cameras see there; camera 0's view of that frame is intact"""
    tm = scene_map()
    obs = RC.exact_block(tm, pair(), RC.bench_poses(6), TAG, 24, pnp_seed=None)
    spoiled = {}
    for i in QC.odd_ids():
        f = gate_frame(i)
        if views_of(obs, i, [f]) == [(f, 0), (f, 1)]:
            QC.spoil(obs[1], f, i, how)
            spoiled[i] = (f, 1)
    assert len(spoiled) >= 3
    return located("gate_per_view_%s_%s" % (how, "on" if gate else "off"), obs, QC.partial_map(QC.odd_ids()), pair(), tm, gate=gate, spoiled=spoiled)


def _gate_cap():
    """id 1: 17 views (9 frames x 2 cameras less the last), 9 of them spoiled at random, one more than the gate may drop;
    id 3: one frame's two views, camera 1's spoiled: the gate never drops the last view"""
    tm = scene_map()
    obs = RC.exact_block(tm, pair(), RC.bench_poses(9), TAG, 24, pnp_seed=None)
    views = views_of(obs, 1)
    assert len(views) == 18
    QC.remove(obs[1], 8, 1)
    rng = np.random.default_rng(11)
    for f, c in views[:17:2]:
        QC.spoil(obs[c], f, 1, "random", rng)
    assert views_of(obs, 3, [0]) == [(0, 0), (0, 1)]
    for f in range(1, 9):
        for c in range(2):
            QC.remove(obs[c], f, 3)
    QC.spoil(obs[1], 0, 3, "shift")
    return located("gate_cap", obs, QC.partial_map([1, 3]), pair(), tm, gate=GATE, views={1: views[:17], 3: [(0, 0), (0, 1)]})


def _sized():
    """odd ids wanted; id SIZED_ID has the side SIZED_SIDE in its entry: both cameras' corners of it are projected at that
    side and its PnP poses are the ones a solve at TAG gives (the true camera<-tag with its translation divided by
    h_id / half)"""
    tm, rig = scene_map(), pair()
    Twr = RC.bench_poses(6)
    obs = RC.exact_block(tm, rig, Twr, TAG, 24, pnp_seed=None)
    h = LR.size_half(SIZED_SIDE, TAG)[0]
    obj = np.array([[-h, -h, 0.0], [h, -h, 0.0], [h, h, 0.0], [-h, h, 0.0]])
    views = views_of(obs, SIZED_ID)
    assert {c for _, c in views} == {0, 1}
    for f, c in views:
        T = rig.cameras[c].T_cam_rig @ np.linalg.inv(Twr[f]) @ tm[SIZED_ID]
        uv = LR.project(LR.camera(rig.cameras[c].K, rig.cameras[c].dist), obj @ T[:3, :3].T + T[:3, 3])
        assert np.all(uv >= 0) and np.all(uv[:, 0] < LC.W) and np.all(uv[:, 1] < LC.H)
        T[:3, 3] /= h / LR.half_size(TAG)
        s = QC.slot_of(obs[c], f, SIZED_ID)
        obs["corners"][c, f, s], obs["T"][c, f, s] = uv.ravel().astype(np.float32), T.ravel()[:12]
    map_in = QC.partial_map(QC.odd_ids())
    map_in["size"][SIZED_ID] = SIZED_SIDE
    return located("sized", obs, map_in, rig, tm)


def _noise():
    tm = scene_map()
    obs = RC.exact_block(tm, pair(), RC.bench_poses(6), TAG, 24, pnp_seed=None)
    rng = np.random.default_rng(7)
    used = (obs["flags"] & 1) != 0
    obs["corners"][used] += rng.normal(0.0, 0.3, obs["corners"][used].shape).astype(np.float32)
    return located("noise", obs, QC.partial_map(QC.odd_ids()), pair(), tm)


BUILDERS = {
    "rear_only": _rear_only,
    "both_cameras": _both_cameras,
    "mixed_models": _mixed_models,
    "frames_edge_63": lambda: _frames_edge(63),
    "frames_edge_64": lambda: _frames_edge(64),
    "frames_edge_65": lambda: _frames_edge(65),
    "frames_edge_130": lambda: _frames_edge(130),
    "views_edge_2": lambda: _views_edge(2),
    "views_edge_15": lambda: _views_edge(15),
    "views_edge_16": lambda: _views_edge(16),
    "views_edge_17": lambda: _views_edge(17),
    "slots_edge_16x16": lambda: _slots_edge(16, 16),
    "slots_edge_8x32": lambda: _slots_edge(8, 32),
    "slots_edge_1x1": _slots_edge_1,
    "gate_cap": _gate_cap,
    "sized": _sized,
    "perturbed": lambda: _side("perturbed", 1),
    "noise": _noise,
}
for _how in QC.SPOILINGS:
    BUILDERS["gate_per_view_%s_on" % _how] = functools.partial(_gate_per_view, _how, GATE)
    BUILDERS["gate_per_view_%s_off" % _how] = functools.partial(_gate_per_view, _how, 0.0)
CASES = sorted(BUILDERS)
RECOVER = ("rear_only", "both_cameras", "mixed_models", "sized")     # the cases whose located tags are held against the truth


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c["name"] == name
    return c


def solo(K, dist):
    """the rig of one camera at the identity: asl_locate_tags_rig_* on obs[None] is asl_locate_tags_* on obs"""
    return Rig([RigCamera(K, dist, np.eye(4))])
