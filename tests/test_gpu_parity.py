"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle, stage by stage.

Bars: bit-exact for every integer/byte/index product (decimated gray, threshold image, component
labels and sizes, tag ids, hamming, corner order); float products (quad corners, detection corners,
margin) are computed with the same IEEE operations in the same order as the oracle, so they are
held to 1e-9 px absolute (observed: identical)."""
import numpy as np
import pytest

import golden_scene as G
import oracle_lib as O
from aprilslam_amd import synth
from stage_check import CORNER_TOL, check_stages, scene_frame

pytestmark = pytest.mark.gpu


def test_default_scene_stage_parity(gpu_detector, family):
    sc = synth.default_scene()
    # camera nudged off the origin so that edges are not pixel-aligned; tags 3 and 4 are outside the 45 deg view
    frame, _ = synth.render_frame(1000, 1000, sc["tags"], 18.0, cam_position=(-0.7, -0.4, 1.1), cam_rotation_deg=(0.5, -1.0, -0.7))
    dets, npf = check_stages(gpu_detector, frame[None], family)
    assert [int(d["id"]) for d in dets] == [0, 1, 2]


@pytest.mark.parametrize("w,h,ntags,seed", [(1280, 720, 20, 1), (640, 480, 6, 2), (1001, 703, 8, 3), (322, 242, 2, 4)])
def test_random_scene_stage_parity(gpu_detector, family, w, h, ntags, seed):
    frame, _ = scene_frame(w, h, ntags, seed)
    dets, npf = check_stages(gpu_detector, frame[None], family)
    if (w, h) == (1280, 720):
        assert len(dets) == ntags and sorted(int(d["id"]) for d in dets) == list(range(ntags))


def test_noisy_batch_stage_parity(gpu_detector, family):
    frames = np.stack([scene_frame(640, 360, 5, 100 + i, noise=3.0)[0] for i in range(4)])
    check_stages(gpu_detector, frames, family)


def test_gray_input_and_empty_frame(gpu_detector, family):
    rng = np.random.default_rng(7)
    frames = np.stack([np.zeros((240, 320), np.uint8), rng.integers(0, 256, (240, 320), dtype=np.uint8),
                       np.full((240, 320), 200, np.uint8)])
    dets, npf = check_stages(gpu_detector, frames, family)
    assert npf[0] == 0 and npf[2] == 0


def test_pnp_parity(gpu_detector, family):
    frame, gt = scene_frame(1280, 720, 20, 11)
    dets, _ = gpu_detector.detect_host(frame)
    K = synth.camera_matrix(1280, 720)
    corners = dets["corners"]
    for dist in (np.zeros(4), np.array([0.05, -0.02, 0.001, -0.0005, 0.01])):
        rv, tv, T, ok = gpu_detector.solve_pnp(corners, K, dist, 10.0)
        orv, otv, oT, ook = O.solve_pnp(corners, K, dist, 10.0)
        assert ok.all() and ook.all()
        # float64 on both sides; libm sin/cos/atan2 differ in the last ulp between host and device
        assert np.abs(tv - otv).max() < 1e-6 and np.abs(rv - orv).max() < 1e-7 and np.abs(T - oT).max() < 1e-6
    # against analytic ground truth: <= 1 mm at 5.56 mm/unit, i.e. 0.18 units, is the north-star bar vs the
    # reference; vs ground truth the detector's corner noise dominates, so only a loose sanity bound here
    rv, tv, T, ok = gpu_detector.solve_pnp(corners, K, np.zeros(4), 10.0)
    for d, t in zip(dets, T):
        g = gt[int(d["id"])]
        assert np.linalg.norm(t[:3, 3] - g[:3, 3]) < 0.02 * np.linalg.norm(g[:3, 3])


def test_device_resident_batch_with_pose(gpu_detector, family):
    import torch
    frames = np.stack([scene_frame(1280, 720, 20, 200 + i)[0] for i in range(3)])
    K = synth.camera_matrix(1280, 720)
    t = torch.from_numpy(frames).to("cuda:0")
    dets, poses, npf = gpu_detector.detect_device(t.data_ptr(), 3, 3, 1280, 720, K=K, dist=np.zeros(4), tag_size=10.0)
    hd, hn = gpu_detector.detect_host(frames)
    assert np.array_equal(npf, hn) and np.array_equal(dets["id"], hd["id"]) and np.array_equal(dets["corners"], hd["corners"])
    rv, tv, T, ok = gpu_detector.solve_pnp(dets["corners"], K, np.zeros(4), 10.0)
    assert np.array_equal(poses["tvec"], tv) and np.array_equal(poses["rvec"], rv) and poses["ok"].all()


def test_tag_detector_detect_carries_the_pose_get_pose_would_compute(family):
    """TagDetector.detect solves the poses in the same submission (asl_detect_batch_pose_u8); get_pose of such a
    detection must return exactly what the stand-alone asl_solve_pnp_batch call returns for its corners."""
    from aprilslam_amd.tag_detector import TagDetector
    frame, _ = scene_frame(1280, 720, 20, 11)
    K = synth.camera_matrix(1280, 720)
    for dist in (np.zeros((4, 1)), np.array([0.05, -0.02, 0.001, -0.0005, 0.01])):
        td = TagDetector({"camera_matrix": K, "dist_coeffs": dist}, tag_size=10.0, id_limit=0)
        dets = td.detect(frame)
        assert len(dets) == 20
        for d in dets:
            ok, rv, tv, T = td.get_pose(d)
            plain = {k: v for k, v in d.items() if k != "_pose"}
            ok2, rv2, tv2, T2 = td.get_pose(plain)
            assert ok == ok2 and np.array_equal(rv, rv2) and np.array_equal(tv, tv2) and np.array_equal(T, T2)
        # a detection whose corners were edited falls back to the stand-alone solve
        e = dict(dets[0]); e["lb-rb-rt-lt"] = dets[0]["lb-rb-rt-lt"] + 1.0
        assert not np.array_equal(td.get_pose(e)[2], td.get_pose(dets[0])[2])
        td.detector._det.close()


def test_only_reference_pinned_ids_by_default(family):
    """A detector decodes ids 0..4 (the ones the reference's tag images pin) unless the build-defined rest of the
    table is opened; the oracle with a 5-entry code book gives the same detections."""
    import copy
    from aprilslam_amd import _lib
    frame, _ = scene_frame(1280, 720, 20, 11)
    det = _lib.Detector("tagStandard41h12")
    dets, _ = det.detect_host(frame)
    fam5 = copy.copy(family)
    fam5.codes = family.codes[:family.pinned_ids]
    ref = O.detect_bgr(frame, fam5)
    assert family.pinned_ids == 5 and sorted(int(d["id"]) for d in dets) == [0, 1, 2, 3, 4]
    assert [int(d["id"]) for d in dets] == [r["id"] for r in ref]
    for d, r in zip(dets, ref):
        assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL
    with pytest.raises(_lib.AslError):
        _lib.check(det._L.asl_detector_set_id_limit(det._h, 100000))
    det.close()


def test_host_rodrigues_matches_device_T(gpu_detector):
    """TagDetector.transformation (host Rodrigues, tag_detector.py:45-52) against the T the PnP kernel returns,
    and the Euler / distance helpers against their closed forms."""
    from aprilslam_amd.tag_detector import TagDetector, rodrigues
    frame, _ = scene_frame(1280, 720, 20, 11)
    dets, _ = gpu_detector.detect_host(frame)
    K = synth.camera_matrix(1280, 720)
    rv, tv, T, ok = gpu_detector.solve_pnp(dets["corners"], K, np.zeros(4), 10.0)
    td = TagDetector.__new__(TagDetector)
    for r, t, Td in zip(rv, tv, T):
        Th = td.transformation(r.reshape(3, 1), t.reshape(3, 1))
        assert np.abs(Th - Td).max() < 1e-12
        assert abs(td.distance(t) - np.sqrt((t ** 2).sum())) < 1e-12
    assert np.array_equal(rodrigues(np.zeros(3)), np.eye(3))
    # yaw about y, pitch about x, roll about z for a pure rotation about one axis
    for axis, idx in ((np.array([0, 1.0, 0]), 0), (np.array([0, 0, 1.0]), 2)):
        e = td.euler_angles(0.3 * axis)
        assert abs(e[idx] - np.degrees(0.3)) < 1e-9 and np.abs(np.delete(e, idx)).max() < 1e-9


def test_pnp_both_minima_option():
    """asl_detector_set_pnp_both_minima: off (default) is the reference's single minimum -- the parity tests above.  On, the
    mirrored planar pose is refined too and the one with the lower reprojection error is kept: per tag the reprojection
    error never gets worse, and on distant tags with noisy corners some poses move to the other minimum.  (Which minimum
    is closer to the truth is a coin toss at that noise level -- the option cannot and does not fix that.)"""
    from aprilslam_amd import _lib
    K = synth.camera_matrix(1280, 720)
    rng = np.random.default_rng(0)
    obj = np.array([(-5, -5, 0.0), (5, -5, 0.0), (5, 5, 0.0), (-5, 5, 0.0)])

    def project(T):
        P = (T[:3, :3] @ obj.T).T + T[:3, 3]
        return np.stack([K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]], axis=1)

    corners = []
    for _ in range(1500):
        T = synth.camera_from_tag([rng.uniform(-30, 30), rng.uniform(-15, 15), -300.0], rng.uniform(-35, 35, 3))
        corners.append(project(T) + rng.normal(0, 0.3, (4, 2)))
    corners = np.array(corners).astype(np.float32).astype(np.float64)
    det = _lib.Detector("tagStandard41h12")
    try:
        cost = {}
        for on in (False, True):
            det.set_pnp_both_minima(on)
            rv, tv, T, ok = det.solve_pnp(corners, K, np.zeros(4), 10.0)
            assert ok.all()
            cost[on] = np.array([((project(T[i]) - corners[i]) ** 2).sum() for i in range(len(corners))])
        assert (cost[True] <= cost[False] + 1e-9).all()
        moved = cost[True] < cost[False] - 1e-9
        assert 5 <= moved.sum() <= 0.2 * len(corners), int(moved.sum())
    finally:
        det.close()


def test_errors_are_loud(gpu_detector):
    from aprilslam_amd import _lib
    with pytest.raises(_lib.AslError):
        _lib.Detector("tag36h11")
    with pytest.raises(_lib.AslError):
        _lib.Detector("tagStandard41h12", decimate=1.5)
    with pytest.raises(_lib.AslError):
        _lib.Detector("tagStandard41h12", blur=0.8)
    img = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError):
        gpu_detector.detect_host(img, K=np.eye(3), dist=np.zeros(3))       # 3 distortion coefficients
    with pytest.raises(_lib.AslError):
        gpu_detector.detect_host(np.zeros((4, 4), np.uint8))               # smaller than the 8x8 minimum
    with pytest.raises(_lib.AslError):
        gpu_detector.detect_device(0, 1, 3, 64, 64)                        # NULL device pointer


def test_gn_backend_matches_cpu_restatement(gpu_detector):
    """Pose-graph LM on the device (MFMA f64 normal blocks) vs oracle/gn_oracle.py: same damping schedule,
    so the iterates agree to rounding; and both recover ground truth on noise-free data."""
    from gn_problem import G, make_problem
    # L = 50 tags: a 300 x 300 reduced system, seven block columns of the blocked Cholesky (MFMA trailing updates, inverse
    # diagonal blocks in the back substitution)
    for seed, noise, P, L in ((3, 0.0, 16, 8), (4, 0.25, 16, 8), (5, 0.25, 24, 50)):
        pr = make_problem(P=P, L=L, seed=seed, noise=noise)
        args = (pr["cam0"], pr["tag0"], pr["obs_cam"], pr["obs_tag"], pr["obs_corners"], pr["K"], 10.0, 0)
        cam_o, tag_o, st_o = G.solve(*args, iters=12)
        cam_g, tag_g, st_g = gpu_detector.gn_solve(*args, iters=12)
        # the number of accepted steps is not compared: once converged, accept / reject is decided by the last bit of the cost
        assert min(st_g[2], st_o[2]) >= 3, (seed, st_g, st_o)
        assert abs(st_g[0] - st_o[0]) <= 1e-9 * st_o[0]
        assert abs(st_g[1] - st_o[1]) <= 1e-6 * max(st_o[1], 1e-9) + 1e-12 * st_o[0]
        assert np.abs(tag_g - tag_o).max() < 1e-6 and np.abs(cam_g - cam_o).max() < 1e-6
        if noise == 0.0:
            assert np.abs(tag_g - pr["tag_gt"]).max() < 1e-6 and np.abs(cam_g - pr["cam_gt"]).max() < 1e-6


def test_gn_backend_full_size_system(gpu_detector):
    """The system of BASELINE.json configs[4]: 24 cameras x 200 tags of a 3840 x 2160 view, ~3,800 observations, a
    1,200 x 1,200 reduced system = 25 block columns of the blocked Cholesky (the shape profiles/r0*_gn_kernel_stats.csv
    profiles).  Same damping schedule on both sides, so the iterates agree to rounding."""
    from gn_problem import G, make_problem
    pr = make_problem(P=24, L=200, seed=6, noise=0.25, width=3840, height=2160)
    assert len(pr["obs_cam"]) > 3000
    args = (pr["cam0"], pr["tag0"], pr["obs_cam"], pr["obs_tag"], pr["obs_corners"], pr["K"], 10.0, 0)
    cam_o, tag_o, st_o = G.solve(*args, iters=6)
    cam_g, tag_g, st_g = gpu_detector.gn_solve(*args, iters=6)
    assert min(st_g[2], st_o[2]) >= 3, (st_g, st_o)
    assert abs(st_g[0] - st_o[0]) <= 1e-9 * st_o[0]
    assert abs(st_g[1] - st_o[1]) <= 1e-6 * st_o[1]
    assert st_g[1] / len(pr["obs_cam"]) < 1.0  # 8 residuals of 0.25 px noise per observation: 0.5 px^2
    assert np.abs(tag_g - tag_o).max() < 1e-6 and np.abs(cam_g - cam_o).max() < 1e-6


@pytest.mark.parametrize("w,h,ntags,seed", [(1920, 1080, 50, 21), (3840, 2160, 200, 22)])
def test_large_config_stage_parity(gpu_detector, family, w, h, ntags, seed):
    """BASELINE.json configs[2] (1080p, 50 tags) and configs[4] (2160p, 200 tags) as single-frame parity cases:
    every stage bit-exact against the oracle, every tag found with its id."""
    frame, _ = scene_frame(w, h, ntags, seed)
    dets, npf = check_stages(gpu_detector, frame[None], family)
    assert sorted(int(d["id"]) for d in dets) == list(range(ntags))


def test_decimate_1_and_maxhamming_variants(family):
    """Non-default detector options (the wrapper's keywords) stay in parity with the oracle."""
    from aprilslam_amd import _lib
    frame, _ = scene_frame(640, 480, 6, 31, noise=2.0)
    for dec, mh, refine in ((1, 1, True), (2, 0, True), (2, 2, False), (3, 1, True)):
        det = _lib.Detector("tagStandard41h12", decimate=float(dec), maxhamming=mh, refine_edges=refine, id_limit=0)
        try:
            dets, _ = det.detect_host(frame)
            gray = O.bgr2gray(frame)
            ref = O.detect_gray(gray, family, dec, mh, 1 if refine else 0)
            assert [int(d["id"]) for d in dets] == [r["id"] for r in ref], (dec, mh, refine)
            for d, r in zip(dets, ref):
                assert int(d["hamming"]) == r["hamming"]
                assert np.abs(d["corners"] - r["corners"]).max() <= CORNER_TOL
        finally:
            det.close()


def test_submit_collect_pipeline_equals_blocking_call(family):
    """Two workspaces used round-robin (submit batch i before collecting batch i-1) give the same results as
    the blocking call, batch by batch."""
    import torch
    from aprilslam_amd import _lib
    K = synth.camera_matrix(640, 360)
    batches = [np.stack([scene_frame(640, 360, 5, 300 + 10 * b + i)[0] for i in range(4)]) for b in range(3)]
    dev = [torch.from_numpy(b).to("cuda:0") for b in batches]
    a, b2 = _lib.Detector(id_limit=0), _lib.Detector(id_limit=0)
    try:
        ref = [a.detect_device(t.data_ptr(), 4, 3, 640, 360, K=K, dist=np.zeros(4), tag_size=10.0) for t in dev]
        ref = [(r[0].copy(), r[1].copy(), r[2].copy()) for r in ref]
        dets = [a, b2]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        got, inflight = [], []
        for i, t in enumerate(dev):
            k = i % 2
            if len(inflight) == 2:
                r = dets[inflight.pop(0)].collect()
                got.append((r[0].copy(), r[1].copy(), r[2].copy()))
            dets[k].submit_device(t.data_ptr(), 4, 3, 640, 360, stream=streams[k].cuda_stream, K=K, dist=np.zeros(4), tag_size=10.0)
            inflight.append(k)
        while inflight:
            r = dets[inflight.pop(0)].collect_view()  # the zero-copy form: views of the detector's own buffers
            got.append((r[0].copy(), r[1].copy(), r[2].copy()))
        for (d0, p0, n0), (d1, p1, n1) in zip(ref, got):
            assert np.array_equal(n0, n1) and np.array_equal(d0["id"], d1["id"]) and np.array_equal(d0["corners"], d1["corners"])
            assert np.array_equal(p0["tvec"], p1["tvec"]) and np.array_equal(p0["rvec"], p1["rvec"])
    finally:
        a.close(); b2.close()


def test_adversarial_textures_grow_buffers_and_stay_in_parity(family):
    """Worst-case inputs for the work buffers: salt-and-pepper blocks, a fine checkerboard (tens of thousands of
    clusters), a tag drowned in noise and one-pixel stripes (the densest boundary there is).  Buffers must grow and re-run (never truncate), results stay bit-exact."""
    from aprilslam_amd import _lib
    rng = np.random.default_rng(99)
    h, w = 360, 640
    noise = (rng.integers(0, 2, (h // 4, w // 4), dtype=np.uint8) * 255).repeat(4, 0).repeat(4, 1)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((((yy // 12) + (xx // 12)) & 1) * 255).astype(np.uint8)
    tagf = O.bgr2gray(scene_frame(w, h, 3, 77, noise=8.0)[0])
    # 2-pixel rows (1 pixel after decimation): ~3 boundary points per pixel, more than a cluster-pass workgroup parks
    # in its small buffer, so these tiles go through the dense-tile launch
    stripes = ((((yy // 2) & 1) * 255)).astype(np.uint8)
    frames = np.stack([noise, checker, tagf, stripes])
    det = _lib.Detector("tagStandard41h12", id_limit=0)
    try:
        dets, npf = check_stages(det, frames, family)
        c = det.debug_counters()
        assert c[11] == 0 and c[12] == 0 and c[13] == 0 and c[14] == 0  # the accepted run had no overflow left
        assert c[16] > 0 and c[17] > 0  # both dense launches had work: the point pass's (stripes) and the labelling pass's (noise)
    finally:
        det.close()


def test_reference_trajectory_on_gpu(gpu_detector, family):
    """The reference's committed run (tests/golden/reference_trajectory.json: 89 pixel-aligned views of the default
    scene, rendered with the reference's own tag images) through the HIP detector + PnP and the graph: stage parity
    against the oracle on the knife-edge frames, and the reference's own logged camera pose (position, Euler angles,
    node count) as the known answer, with the same bars as the oracle (tests/golden_scene.py)."""
    frames = np.stack([G.render(G.camera_position(r))[0] for r in G.TRAJ])
    check_stages(gpu_detector, frames[[0, 7, 15, 33, 35, 63, 71, 80, 88]], family)
    dets, npf = gpu_detector.detect_host(frames)
    rv, tv, T, ok = gpu_detector.solve_pnp(dets["corners"], G.K, np.zeros(4), G.TAG_SIZE)
    assert ok.all()
    slam = G.new_slam()
    start, poses, ids, nodes = 0, [], [], []
    for b in range(len(G.TRAJ)):
        sl = slice(start, start + npf[b])
        start += npf[b]
        ids.append([int(i) for i in dets["id"][sl]])
        poses.append(G.feed(slam, ids[-1], T[sl]))
        nodes.append(len(slam.graph.get_nodes()))
    d_ref, d_rpy = G.check_trajectory(poses, ids, nodes)
    assert d_ref[0] < 0.02


@pytest.mark.parametrize("maxhamming", [0, 1, 2, 3])
def test_code_book_index_with_damaged_payloads(family, maxhamming, monkeypatch):
    """Tags whose payload has 0..4 flipped cells, decoded with every maxhamming: the code-book index of k_decode (a word
    within maxhamming of a code shares one of maxhamming + 1 bit chunks with it) against the oracle's search of the whole
    book, and against the device's own whole-book search (ASL_NO_CODE_INDEX)."""
    from aprilslam_amd import _lib
    from aprilslam_amd.families import get_family
    fam = get_family("tagStandard41h12")
    rng = np.random.default_rng(77 + maxhamming)
    w, h = 1280, 720
    tags = synth.random_scene(w, h, 12, np.random.default_rng(5))
    textures = {}
    flips = {}
    off = (fam.total_width - fam.width_at_border) // 2
    for k, t in enumerate(tags):
        g = fam.grid(t["id"]).copy()
        nflip = k % 5
        for i in rng.choice(fam.nbits, size=nflip, replace=False):
            g[fam.bit_y[i] + off, fam.bit_x[i] + off] ^= 1
        flips[t["id"]] = nflip
        textures[t["id"]] = np.repeat((np.kron(g, np.ones((40, 40), dtype=np.uint8)) * 255)[:, :, None], 3, axis=2)
    frame, _ = synth.render_frame(w, h, tags, 18.0, textures=textures)
    ref = O.detect_gray(O.bgr2gray(frame), family, 2, maxhamming=maxhamming)
    results = []
    for no_index in (False, True):
        if no_index:
            monkeypatch.setenv("ASL_NO_CODE_INDEX", "1")
        det = _lib.Detector("tagStandard41h12", decimate=2.0, id_limit=0, maxhamming=maxhamming)
        try:
            dets, _, npf = det.detect_host(frame[None], K=synth.camera_matrix(w, h), dist=np.zeros(4), tag_size=10.0)
            results.append([(int(d["id"]), int(d["hamming"])) for d in dets])
        finally:
            det.close()
    assert results[0] == results[1] == [(r["id"], r["hamming"]) for r in ref]
    seen = dict(results[0])
    for tid, nflip in flips.items():
        if nflip <= maxhamming:
            assert seen.get(tid) == nflip, (tid, nflip, seen.get(tid))
    assert max(hm for _, hm in results[0]) == min(maxhamming, 4)
