#!/usr/bin/env python3
"""Record tests/golden/localize_statements.npz: what the NumPy statements of the solvers that take a tag map and solve one
pose at a time (tests/localize_ref.py with tests/rig_ref.py, tests/calib_ref.py, tests/locate_ref.py, and tests/sized_ref.py
over the first three) returned before localize_ref.py and calib_ref.py honoured per-tag sizes themselves.

Recorded at commit 15d424c ("Locate unmapped tags from posed frames: extend a tag map on the device"), the last one that
has sized_ref.py: there localize_ref and calib_ref fixed one tag_size, and sized_ref restated five of their functions with
the size rule and put them over the originals (its context manager honoured()) while a sized call ran.  The recorder
imports everything (cases, statements, package) from a checkout of that commit and runs on the CPU only:

    git worktree add --detach /tmp/parent 15d424c
    python tests/golden/make_localize_statement_fixtures.py record /tmp/parent/tests     # writes localize_statements.npz
    python tests/golden/make_localize_statement_fixtures.py compare                      # today's statements against the record

runs() is the list of recorded calls, built from the cases modules on sys.path; tests/test_localize_statement_golden.py runs
the same list through today's statements and compare() states what must be equal.  Every run is recorded by the statement
that owned its call: the sets "camera", "rig", "calib" and "locate" by localize_ref, rig_ref, calib_ref and locate_ref as they
were, the set "sized" through sized_ref's fronts (localize, localize_rig, calibrate).  The calls are those the CPU statement
tests and the device comparisons make on the cases modules, at their own gate, sigma_px, n_dist, flags and max_iters; a
localisation is always recorded with its traces, and with a covariance where a test asks for one (the poses of a call with
sigma_px are the bytes of the call without).  Left out, as repeats of a recorded code path on other random corners: the 200
and 500 noisy draws of test_rig_ref's scatter tests and the 100 of test_calib_ref's (the recorded "calib/dense_*" runs are
noisy calibrations of the same scenes), and calls on blocks that only a detector produces.

The file (the key list "layout" says the same): "keys", the runs' names; "names", the fields a run can have; "lens"
(runs x names), how many values of each field a run has; then every field over the runs end to end, the integer ones as
int32 (the map's float32 sizes as their bit patterns), the doubles as eight byte planes of their bit patterns, so every
double is the recorded one exactly.  Trace lists of varying length are laid end to end with their lengths in "trace.lens".
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "localize_statements.npz")
SETS = ("camera", "rig", "calib", "locate", "sized")
# the doubles that are compared by their largest relative difference; every other field byte for byte
LOOSE = {"poses.rms_px", "poses.rms_seed_px", "res.K", "res.dist", "res.std", "res.rms_px", "res.rms_init_px", "fit.rms_px", "fit.rms_seed_px"}
NOISE_SEED, NOISE_PX = 11, 0.2            # test_gpu_pose_cov.noisy


def runs():
    """(key, set name, kind, args, kwargs) of every recorded call.  kind "cam": args (obs (F, S), map, K, dist, tag_size); "rig":
    (obs (C, F, S), map, rig, tag_size); both with kwargs max_tag_rms_px, sigma_px.  "cal": (obs, map, tag_size, width, height),
    kwargs of calibrate.  "locate": locate_tags' (obs, poses, map, K, dist, tag_size, gate, min_views), kwargs sigma_px."""
    import calib_cases as CC
    import calib_ref as CR
    import localize_cases as LC
    import locate_cases as QC
    import rig_cases as RC
    import sized_cases as ZC
    import solver_edge_cases as E
    from aprilslam_amd.rig import Rig, RigCamera

    out = []
    K, TAG = ZC.K, LC.TAG_INNER

    def noisy(obs, px, seed):
        o = obs.copy()
        o["corners"] = (obs["corners"].astype(np.float64) + np.random.default_rng(seed).normal(scale=px, size=obs["corners"].shape)).astype(np.float32)
        return o

    # camera: localize_cases and the localisation edge cases, given sigma (the sized-ref tests' and test_gpu_pose_cov's 0.5) and,
    # on test_gpu_pose_cov's noisy copies, the estimated one
    for name, obs, rec, dist, gate in list(LC.cpu_cases(K)) + [c[:5] for c in E.loc_cases()]:
        a = (obs, rec, K, dist, TAG)
        out.append(("camera/%s/s0.5" % name, "camera", "cam", a, dict(max_tag_rms_px=gate, sigma_px=0.5)))
        out.append(("camera/%s/noisy/s0" % name, "camera", "cam", (noisy(obs, NOISE_PX, NOISE_SEED),) + a[1:], dict(max_tag_rms_px=gate, sigma_px=0.0)))
    # rig: rig_cases as test_gpu_rig and test_rig_ref call them; the two status blocks; the moved rig frame; one camera at the identity
    for c in RC.cases():
        out.append(("rig/%s/s0.5" % c["name"], "rig", "rig", (c["obs"], c["rec"], c["rig"], c["tag_size"]), dict(max_tag_rms_px=c["gate"], sigma_px=0.5)))
    c = RC.case("side_by_side")
    obs = c["obs"].copy()
    obs["flags"][:, 0] = 0
    obs["flags"][:, 1] &= 1
    out.append(("rig/statuses/s0.5", "rig", "rig", (obs, c["rec"], c["rig"], c["tag_size"]), dict(sigma_px=0.5)))
    obs = noisy(c["obs"], 0.2, 12)
    obs["flags"][:, 0] = 0
    obs["flags"][:, 1] &= 1
    out.append(("rig/statuses/noisy/s0", "rig", "rig", (obs, c["rec"], c["rig"], c["tag_size"]), dict(sigma_px=0.0)))
    Di = np.linalg.inv(RC.transform((0.3, -0.5, 0.2), (3.0, -1.5, 2.0)))
    for name in ("side_by_side", "back_to_back", "mixed_models", "gate"):
        c = RC.case(name)
        moved = Rig([RigCamera(rc.K, rc.dist, rc.T_cam_rig @ Di) for rc in c["rig"].cameras])
        out.append(("rig/%s/moved" % name, "rig", "rig", (c["obs"], c["rec"], moved, c["tag_size"]), dict(max_tag_rms_px=c["gate"])))
    for name, obs, rec, dist, gate in LC.cpu_cases(K):
        out.append(("rig/identity/%s" % name, "rig", "rig", (obs[None], rec, Rig([RigCamera(K, dist, np.eye(4))]), TAG), dict(max_tag_rms_px=gate)))
    # calib: calib_cases.cpu_cases, test_calib_ref's own calls on calib_cases' scenes, sized_ref's test call, the edge cases
    def cal(key, obs, rec, kw, name="calib"):
        out.append((name + "/" + key, name, "cal", (obs, rec, TAG, CC.W, CC.H), kw))

    for name, obs, rec, kw in CC.cpu_cases():
        cal(name, obs, rec, kw)
    sc, rec, _ = CC.scene_case()
    bd, brec, _ = CC.board_case()
    cal("board5", bd, brec, dict(n_dist=5))
    cal("scene4", CC.scene_case(dist=CC.DIST4)[0], rec, dict(n_dist=4))
    cal("scene4/pinhole", CC.scene_case(dist=CC.DIST4)[0], rec, dict(n_dist=0))
    cal("scene5/pinhole", sc, rec, dict(n_dist=0))
    K0 = CC.K_TRUE + np.array([[5.0, 0, 3.5], [0, -4.0, -2.25], [0, 0, 0]])
    cal("flags/fix_pp", sc, rec, dict(n_dist=5, K_init=K0, flags=CR.FIX_PRINCIPAL_POINT))
    cal("flags/fix_aspect", sc, rec, dict(n_dist=5, K_init=K0, flags=CR.FIX_ASPECT_RATIO))
    cal("flags/zero_tangent", CC.board_case(dist=CC.DIST4)[0], brec, dict(n_dist=4, flags=CR.ZERO_TANGENT_DIST))
    cal("flags/all", sc, rec, dict(n_dist=5, flags=7))
    for tname, o in (("scene", sc), ("board", bd)):
        o = o.copy()
        o["corners"] += np.random.default_rng(1).normal(0, 0.2, o["corners"].shape).astype(np.float32) * (o["id"] >= 0)[..., None]
        for kname, kw in (("d5", dict(n_dist=5)), ("d4_flags", dict(n_dist=4, flags=CR.FIX_ASPECT_RATIO | CR.ZERO_TANGENT_DIST))):
            cal("dense_%s_%s" % (tname, kname), o, rec if tname == "scene" else brec, kw)
    fr = CC.board_case(n=6, fronto=True)[0]
    cal("fronto/K_init", fr, brec, dict(n_dist=5, K_init=CC.K_TRUE, flags=CR.FIX_PRINCIPAL_POINT))
    cal("fronto/d0_i4", fr, brec, dict(n_dist=0, max_iters=4))
    for name, obs, rec, kw, _ in E.cal_cases():
        cal("edges/" + name, obs, rec, kw)
    # locate: every case without and with the covariance (test_gpu_locate: sigma 0); the noise case also at a given sigma
    for name in QC.CASES:
        _, obs, poses, map_in, dist, gate, min_views = QC.case(name)
        for key, sig in (("plain", None), ("s0", 0.0)) + ((("s0.5", 0.5),) if name == "noise" else ()):
            out.append(("locate/%s/%s" % (name, key), "locate", "locate", (obs, poses, map_in, QC.K, dist, QC.TAG, gate, min_views), dict(sigma_px=sig)))
    # sized: sized_cases through sized_ref
    for mt in ZC.LOC_MAX_TAGS:
        obs, rec, dist, _ = ZC.loc_case(mt)
        out.append(("sized/loc%d" % mt, "sized", "cam", (obs, rec, K, dist, ZC.TAG), dict(max_tag_rms_px=ZC.GATE, sigma_px=ZC.SIGMA)))
    obs, rec, dist, _ = ZC.loc_case(2)
    for bname, bad in (("negative", -1.0), ("nan", np.nan), ("inf", np.inf)):
        for ids in ([1], [1, 16]):                  # test_sized_ref's and test_gpu_sized's substitutions
            a, b = rec.copy(), rec.copy()
            a["size"][ids] = bad
            b["valid"][ids] = 0
            for how, m in (("size", a), ("valid", b)):
                out.append(("sized/bad_%s/%s%s" % (bname, how, ids), "sized", "cam", (obs, m, K, dist, ZC.TAG), dict(sigma_px=ZC.SIGMA)))
    obs, rec, rig = ZC.rig_case()
    out.append(("sized/rig", "sized", "rig", (obs, rec, rig, ZC.TAG), dict(max_tag_rms_px=0.0, sigma_px=ZC.SIGMA)))
    for sized in (True, False):
        obs, rec, _ = ZC.truth_case(sized)
        out.append(("sized/truth/%s" % ("sized" if sized else "equal"), "sized", "cam", (obs, rec, K, None, ZC.TAG), dict()))
    obs, rec, _ = ZC.truth_case()
    out.append(("sized/truth/sizes_dropped", "sized", "cam", (obs, ZC.without_sizes(rec), K, None, ZC.TAG), dict()))
    (a, rec_a), (b, rec_b) = ZC.uniform_case(10.0, 25.0)
    out.append(("sized/uniform/a", "sized", "cam", (a, rec_a, K, None, 10.0), dict()))
    out.append(("sized/uniform/b", "sized", "cam", (b, rec_b, K, None, 25.0), dict()))
    for n_dist in (0, 5):
        obs, rec = ZC.calib_case(n_dist)
        cal("calib/d%d" % n_dist, obs, rec, dict(n_dist=n_dist), name="sized")
    return out


def run_one(run, sized_ref=None):
    """the call through the statements on sys.path -> the statement's outputs and its traces; sized_ref: the module whose fronts
    a run of the set "sized" goes through (the recorded commit's), None: the statements themselves"""
    import calib_ref as CR
    import localize_ref as LR
    import locate_ref as QR
    import rig_ref as RR
    _, name, kind, args, kw = run
    front = sized_ref if name == "sized" else None
    if kind == "cal":
        return (front.calibrate if front else CR.calibrate)(*args, **kw), None
    traces = {} if kind == "locate" else []
    if kind == "locate":
        return QR.locate_tags(*args, traces=traces, **kw), traces
    fn = {"cam": front.localize if front else LR.localize, "rig": front.localize_rig if front else RR.localize}[kind]
    return fn(*args, traces=traces, **kw), traces


def ragged(lists, dtype):
    """lists laid end to end, and their lengths"""
    lists = [np.asarray(x, dtype=dtype).ravel() for x in lists]
    return (np.concatenate(lists) if lists else np.zeros(0, dtype=dtype)), [len(x) for x in lists]


def fields(kind, result):
    """{field: its values, flat; float64 for the doubles, int32 otherwise} of a run's outputs"""
    out, traces = result
    f, lens = {}, []
    if kind == "locate":
        f["map.T"], f["map.valid"], f["map.size"] = out[0]["T"], out[0]["valid"], np.ascontiguousarray(out[0]["size"]).view(np.int32)
        fit = out[1]
        f.update({"fit." + k: fit[k] for k in fit.dtype.names})
        cov = out[2] if len(out) == 3 else None
        ids = sorted(traces)
        f["trace.ids"] = np.array(ids, dtype=np.int64)
        f["trace.dropped"], n = ragged([traces[i][1]["dropped"] for i in ids], np.int64)
        first = [traces[i][1]["first"] for i in ids]
        f["trace.first"] = ragged([[(v, m) for v, m, _ in x] for x in first], np.int64)[0]
        f["trace.first_score"], m = ragged([[c for _, _, c in x] for x in first], np.float64)
        f["trace.active"] = ragged([traces[i][3] for i in ids], np.int64)[0]
        lens = n + m + [len(traces[i][3]) for i in ids]
    else:
        if kind == "cal":
            res, poses, cov = out[0], out[1], None
            f.update({"res." + k: res[k] for k in res.dtype.names})
        else:
            poses, cov = out if isinstance(out, tuple) else (out, None)
            for k in ("top_k", "dropped", "active"):
                f["trace." + k], n = ragged([t[k] for t in traces], np.int64)
                lens += n
            f["trace.gate_rms"], n = ragged([np.concatenate(t["gate_rms"]) if t["gate_rms"] else [] for t in traces], np.float64)
            lens += n + [len(t["gate_rms"]) for t in traces]
        f.update({"poses." + k: poses[k] for k in poses.dtype.names})
    if cov is not None:
        f.update({"cov." + k: cov[k] for k in cov.dtype.names})
    f["trace.lens"] = np.array(lens, dtype=np.int64)
    done = {}
    for k, a in f.items():
        a = np.asarray(a)
        done[k] = np.ascontiguousarray(a, dtype=np.float64).ravel() if a.dtype == np.float64 else a.astype(np.int32).ravel()
        assert a.dtype == np.float64 or np.array_equal(done[k], a.ravel()), k
    return done


def save(path, arrays):
    """an .npz (np.load reads it) whose members are LZMA-compressed"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as zf:
        for k, a in arrays.items():
            with zf.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def pack(recorded):
    """recorded: [(run, fields)] in runs() order -> the arrays of the file"""
    names = list(dict.fromkeys(k for _, f in recorded for k in f))
    dbl = {k: any(f[k].dtype == np.float64 for _, f in recorded if k in f) for k in names}
    arrays = dict(keys=np.array([r[0] for r, _ in recorded]), names=np.array(names),
                  lens=np.array([[len(f.get(k, ())) for k in names] for _, f in recorded], dtype=np.int32))
    for k in names:
        a = np.concatenate([f[k] for _, f in recorded if k in f])
        assert a.dtype == (np.float64 if dbl[k] else np.int32), k
        arrays[k] = np.ascontiguousarray(a.view(np.uint8).reshape(-1, 8).T) if dbl[k] else a        # byte planes, (8, n)
    arrays["layout"] = np.array(["keys", "names", "lens (runs x names)"] + names + ["layout"])
    return arrays


def load(path=OUT):
    """{key: {field: values, flat}} with every double as it was recorded; a field a run does not have is absent"""
    z = dict(np.load(path))
    names = [str(k) for k in z["names"]]
    for k in names:
        if z[k].dtype == np.uint8:
            z[k] = np.ascontiguousarray(z[k].T).view(np.float64).ravel()
    at = dict.fromkeys(names, 0)
    out = {}
    for key, lens in zip(z["keys"], z["lens"]):
        e = {}
        for k, n in zip(names, lens):
            if n or k == "trace.lens":
                e[k] = z[k][at[k]:at[k] + n]
                at[k] += n
        out[str(key)] = e
    assert all(at[k] == len(z[k]) for k in names)
    return out


def rel(a, b):
    """0 if the bytes are equal; else the largest |a - b| / |b| over the entries (where the record b is 0, a must be 0)"""
    if a.tobytes() == b.tobytes():
        return 0.0
    assert a.shape == b.shape and np.array_equal(a[b == 0], b[b == 0]) and np.array_equal(np.isfinite(a), np.isfinite(b))
    nz = (b != 0) & np.isfinite(b)
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


def compare(key, e, cur):
    """a run's fields cur against its record e.  Asserts what must be equal: the same fields, and byte for byte every integer
    field (counts, statuses, seed_slot, every trace list), every T, every covariance entry with its sigma, the gate's RMS
    and the locate candidates' scores.  Returns the largest relative difference of the doubles of LOOSE and the field it is at."""
    cur = {k: v for k, v in cur.items() if len(v) or k == "trace.lens"}
    assert sorted(cur) == sorted(e), (key, sorted(cur), sorted(e))
    worst = (0.0, "")
    for k in cur:
        if k in LOOSE:
            worst = max(worst, (rel(cur[k], e[k]), k))
        else:
            assert cur[k].dtype == e[k].dtype and cur[k].tobytes() == e[k].tobytes(), (key, k)
    return worst


def main(argv):
    if argv[:1] == ["record"] and len(argv) == 2:
        parent = os.path.abspath(argv[1])
        sys.path[:0] = [parent, os.path.dirname(parent)]
        import sized_ref
        recorded = []
        for run in runs():
            recorded.append((run, fields(run[2], run_one(run, sized_ref))))
            print(run[0], flush=True)
        save(OUT, pack(recorded))
        back = load()
        assert list(back) == [r[0] for r, _ in recorded]
        for run, f in recorded:
            assert compare(run[0], back[run[0]], f)[0] == 0.0, run[0]
        print("%d runs, %d bytes" % (len(recorded), os.path.getsize(OUT)))
    elif argv == ["compare"]:
        sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
        rec = load()
        todo = runs()
        assert [r[0] for r in todo] == list(rec)
        for name in SETS:
            worst = (0.0, "", "")
            for run in [r for r in todo if r[1] == name]:
                worst = max(worst, compare(run[0], rec[run[0]], fields(run[2], run_one(run))) + (run[0],))
            print("%s: largest relative difference %.3g%s over %d runs" % (name, worst[0], " (%s of %s)" % worst[1:] if worst[0] else "",
                                                                           sum(r[1] == name for r in todo)), flush=True)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
