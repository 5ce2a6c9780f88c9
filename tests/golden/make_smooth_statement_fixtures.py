#!/usr/bin/env python3
"""Record tests/golden/smooth_statements.npz: what the NumPy statements of the sequence localisation (tests/smooth_ref.py,
its timed and rig copies tests/smooth_timed_ref.py and tests/smooth_rig_ref.py, tests/smooth_cov_ref.py, and tests/sized_ref.py
over them) returned before they became the one statement tests/smooth_ref.py with tests/smooth_cov_ref.py.

Recorded at commit 3db73a4 ("Tag-map reconstruction: one NumPy statement, one map call path in _lib"), the last one that
has the copies.  The recorder imports everything (cases, statements, package) from a checkout of that commit and runs on
the CPU only:

    git worktree add --detach /tmp/parent 3db73a4
    python tests/golden/make_smooth_statement_fixtures.py record /tmp/parent/tests     # writes smooth_statements.npz
    python tests/golden/make_smooth_statement_fixtures.py compare                      # the one statement against the record

runs() is the list of recorded calls, built from the cases modules on sys.path; tests/test_smooth_statement_golden.py runs
the same list through the one statement and compare() states what must be equal.  Every run is recorded by the statement
that owned its call: a single-camera call without times by smooth_ref (its covariance by smooth_cov_ref), one with times
or of several sequences by the timed copy, a rig's by the rig copy, the sized cases through sized_ref; each at the huber_px
and max_iters its tests use, plain and with reverse=True where a test makes that call: smooth_cases at huber 0 (at the
robust tests' threshold no test reverses them), the robust, timed and sized cases, the rig cases at the compared trials
(reversal_error; at MAX_ITERS no test reverses them).  A covariance run solves first and records the covariance at the
poses and result of that solve.

The file (the key list "layout" says the same): per run the number of frames, of result records, of posed frames and of
trials and whether it has a covariance and a trace; then every field of FIELDS over the runs end to end, the integer ones as
int32, the doubles as eight byte planes of their bit patterns.  The doubles of a reverse=True run are stored as the int64
difference of their bit patterns from the plain run before it wherever the two have the same length, which is a few last
bits and so compresses, and a plain run's T as the difference from third_row(); load() undoes all three, so every double is
the recorded one exactly.  A covariance is stored as its lower triangle (the recorder asserts that it is symmetric to the
bit, and so does compare()).  With all of that the file is 453 KB; the per-trial costs of the reversed runs are in it.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "smooth_statements.npz")
POSE_F8, POSE_I4 = ("T", "rms_px", "rms_seed_px"), ("n_tags", "n_rejected", "status", "seed_slot")
RES_F8, RES_I4 = ("cost_seed", "cost", "rms_px", "rms_seed_px"), ("n_frames_data", "n_filled", "n_flipped", "iterations", "status", "n_soft", "reserved")
TRIL = np.tril_indices(6)
# (field, is a double, doubles or ints per frame / result record / frame with a covariance / posed frame / trial)
FIELDS = ([("poses." + k, True, (16 if k == "T" else 1, 0, 0, 0, 0)) for k in POSE_F8] + [("poses." + k, False, (1, 0, 0, 0, 0)) for k in POSE_I4] +
          [("res." + k, True, (0, 1, 0, 0, 0)) for k in RES_F8] + [("res." + k, False, (0, 2 if k == "reserved" else 1, 0, 0, 0)) for k in RES_I4] +
          [("cov.cov", True, (0, 0, 21, 0, 0)), ("cov.sigma_px", True, (0, 0, 1, 0, 0)), ("cov.dof", False, (0, 0, 1, 0, 0)),
           ("cov.status", False, (0, 0, 1, 0, 0)), ("trace.posed", False, (0, 0, 0, 1, 0)), ("trace.choice", False, (0, 0, 0, 1, 0)),
           ("trace.d", True, (0, 0, 0, 2, 0)), ("trace.tr", True, (0, 0, 0, 4, 0)), ("trace.cost", True, (0, 0, 0, 0, 1))])
LAYOUT = ("keys", "dims (n_frames, n_results, has cov, has trace, n_posed, n_trials, n_choice)",
          "delta (one row per run, one column per double field; 1: int64 differences from the run before)") + tuple(f[0] for f in FIELDS) + ("layout",)
SETS = ("plain", "robust", "seq", "cov", "timed", "rig", "sized")


def runs():
    """(key, set name, kind, args, kwargs) of every recorded call.  kind "cam": args (obs (F, S), map, K, dist, tag_size, seed,
    sigmas, max_iters); "rig": args (obs (C, F, S), map, rig, tag_size, seed, sigmas, max_iters); "cam_seq" / "rig_seq": seq_start
    after obs; "cam_cov" / "rig_cov": the solve's args, the covariance at its output; "sized_": the same through sized_ref.
    kwargs: times, huber_px, reverse.  A reverse=True run follows its plain run."""
    import sized_cases as ZC
    import smooth_cases as SC
    import smooth_cov_cases as VC
    import smooth_rig_cases as GC
    import smooth_robust_cases as RC
    import smooth_seq_cases as SQ
    import smooth_timed_cases as TC

    def both(key, name, kind, args, kw):
        return [(key + "/fwd", name, kind, args, kw), (key + "/rev", name, kind, args, dict(kw, reverse=True))]

    def cam(obs, rec, seed, dist, sig, iters):
        return (obs, rec, SC.K, dist, SC.TAG, seed, sig, iters)

    def seq(b):
        return (b.obs, b.seq_start, b.rec, SC.K, b.dist, SC.TAG, b.seed, b.sigmas, b.max_iters)

    out = []
    # plain: smooth_cases at huber 0, plain and reversed, and at the robust tests' threshold; the failure cases
    for n, obs, rec, seed, dist, sig, iters in SC.all_cases():
        out += both("plain/%s/h0" % n, "plain", "cam", cam(obs, rec, seed, dist, sig, iters), dict(huber_px=0.0))
        out.append(("plain/%s/h%g" % (n, RC.SHAPE_HUBER), "plain", "cam", cam(obs, rec, seed, dist, sig, iters), dict(huber_px=RC.SHAPE_HUBER)))
    for n, (obs, rec, seed, sig, iters, _, _) in SC.failure_cases().items():
        out += both("plain/%s/h0" % n, "plain", "cam", cam(obs, rec, seed, None, sig, iters), dict(huber_px=0.0))
    # robust: its shapes and the scene
    for n, obs, rec, seed, dist, sig, hub, iters in RC.all_cases():
        out += both("robust/%s/h%g" % (n, hub), "robust", "cam", cam(obs, rec, seed, dist, sig, iters), dict(huber_px=hub))
    # seq: the batches through smooth_sequences
    for n, b in (("ragged1", SQ.ragged(1)), ("ragged4", SQ.ragged(4)), ("ragged_dist", SQ.ragged_dist()), ("stop_apart", SQ.stop_apart()),
                 ("failures", SQ.failures()), ("short_pattern", SQ.short_pattern()), ("many_short", SQ.many_short()),
                 ("robust_ragged", RC.ragged()), ("robust_mixed", RC.mixed())):
        out.append(("seq/%s" % n, "seq", "cam_seq", seq(b), dict(huber_px=b.huber)))
    # cov
    for n in VC.DEVICE_CASES + VC.NO_SOLVE_CASES + ["prior_only"]:
        out.append(("cov/%s" % n, "cov", "cam_cov", cam(*(VC.prior_only() if n == "prior_only" else VC.case(n))), dict(huber_px=0.0)))
    # timed: its cases, the batches, the one robust sequence the device comparison makes, the gap scene with its covariance
    for n, obs, rec, seed, dist, times, sig, iters in TC.all_cases():
        out += both("timed/%s" % n, "timed", "cam", cam(obs, rec, seed, dist, sig, iters), dict(times=times))
    for n, (b, times) in (("ragged1", TC.ragged(1)), ("ragged4", TC.ragged(4)), ("bad_times", TC.bad_times_batch())):
        out.append(("timed/seq_%s" % n, "timed", "cam_seq", seq(b), dict(times=times)))
    b, times = TC.ragged(4)
    a0, a1 = SQ.ranges(b)[3]
    out.append(("timed/ragged4[3]/h%g" % RC.SHAPE_HUBER, "timed", "cam", cam(b.obs[a0:a1], b.rec, b.seed[a0:a1], None, b.sigmas, b.max_iters),
                dict(times=times[a0:a1], huber_px=RC.SHAPE_HUBER)))
    obs, rec, seed, _ = TC.gap_scene()
    k = TC.kept_frames()
    kept = cam(obs[k], rec, seed[k], None, TC.GAP_SIGMAS, SC.MAX_ITERS)
    eo, _, es = TC.emptied_gap()
    out.append(("timed/gap", "timed", "cam", kept, dict(times=k.astype(np.float64))))
    out.append(("timed/gap_naive", "timed", "cam", kept, dict()))
    out.append(("timed/gap_emptied", "timed", "cam", cam(eo, rec, es, None, TC.GAP_SIGMAS, SC.MAX_ITERS), dict()))
    out.append(("timed/cov_gap", "timed", "cam_cov", kept, dict(times=k.astype(np.float64))))
    # rig: every case at its own trials and at the compared ones, the sequences, the covariance cases
    for n, obs, rec, rig, seed, sig, iters, times in GC.all_cases():
        for hub in (0.0, GC.HUBER_PX):
            for it in sorted({iters, GC.COMPARE_ITERS}, reverse=True):
                run = both("rig/%s/h%g/i%d" % (n, hub, it), "rig", "rig", (obs, rec, rig, GC.TAG, seed, sig, it), dict(times=times, huber_px=hub))
                out += run if it == GC.COMPARE_ITERS else run[:1]
    obs, rec, rig, seed = GC.three_sequences()
    for hub in (0.0, GC.HUBER_PX):
        out.append(("rig/three_sequences/h%g" % hub, "rig", "rig_seq", (obs, GC.SEQ_START, rec, rig, GC.TAG, seed, GC.SHAPE_SIGMAS, GC.COMPARE_ITERS),
                    dict(huber_px=hub)))
    for n, hub in (("shape3_5_64", 0.0), ("gap", 0.0), ("mixed_models", GC.HUBER_PX)):
        _, obs, rec, rig, seed, sig, iters, times = GC.case(n)
        out.append(("rig/cov_%s/h%g" % (n, hub), "rig", "rig_cov", (obs, rec, rig, GC.TAG, seed, sig, iters), dict(times=times, huber_px=hub)))
    # sized
    obs, rec, seed = ZC.smooth_case()
    args = (obs, rec, ZC.K, None, ZC.TAG, seed, ZC.SMOOTH_SIGMAS, ZC.SMOOTH_ITERS)
    for hub in (0.0, 0.3):
        out += both("sized/smooth/h%g" % hub, "sized", "sized_cam", args, dict(huber_px=hub))
    out.append(("sized/cov", "sized", "sized_cam_cov", args, dict()))
    obs, rec, rig, seed = ZC.smooth_rig_case()
    out += both("sized/rig", "sized", "sized_rig", (obs, rec, rig, ZC.TAG, seed, ZC.SMOOTH_SIGMAS, ZC.SMOOTH_ITERS), dict())
    return out


def run_parent(run):
    """the call through the statement that owned it at the recorded commit -> (poses, results, covariance or None, trace or None)"""
    import sized_ref as ZR
    import smooth_cov_ref as SV
    import smooth_ref as SR
    import smooth_rig_ref as SG
    import smooth_timed_ref as ST
    _, _, kind, args, kw = run
    kw = dict(kw)
    times = kw.pop("times", None)
    sig, iters = args[-2:]
    a = args[:-2]
    if kind == "cam":
        out, res, trace = SR.smooth(*a, *sig, iters, **kw) if times is None else ST.smooth(*a, times, *sig, iters, **kw)
        return out, res, None, trace
    if kind == "cam_seq":
        return ST.smooth_sequences(*a, times, *sig, iters, **kw) + (None, None)
    if kind == "cam_cov":
        if times is None:
            out, res, _ = SR.smooth(*a, *sig, iters, **kw)
            return out, res, SV.smooth_cov(*a[:5], out, res, *sig, **kw), None
        out, res, _ = ST.smooth(*a, times, *sig, iters, **kw)
        return out, res, ST.smooth_cov(*a[:5], out, res, times, *sig, **kw)[0], None
    if kind == "rig":
        out, res, trace = SG.smooth(*a, *sig, iters, times=times, **kw)
        return out, res, None, trace
    if kind == "rig_seq":
        return SG.smooth_sequences(*a, *sig, iters, times=times, **kw) + (None, None)
    if kind == "rig_cov":
        out, res, _ = SG.smooth(*a, *sig, iters, times=times, **kw)
        return out, res, SG.smooth_cov(*a[:4], out, res, *sig, times=times, **kw)[0], None
    return run_sized(ZR, kind, a, times, sig, iters, kw)


def run_sized(ZR, kind, a, times, sig, iters, kw):
    """the sized fronts of the recorded commit's sized_ref"""
    if kind == "sized_cam":
        out, res, trace = ZR.smooth(*a, times, *sig, iters, **kw)
        return out, res, None, trace
    if kind == "sized_cam_cov":
        out, res, _ = ZR.smooth(*a, times, *sig, iters, **kw)
        return out, res, ZR.smooth_cov(*a[:5], out, res, times, *sig, **kw)[0], None
    assert kind == "sized_rig", kind
    out, res, trace = ZR.smooth_rig(*a, *sig, iters, times=times, **kw)
    return out, res, None, trace


def run_one(run):
    """the call through the one statement -> (poses, results, covariance or None, trace or None); a sized run is the same call:
    the statements honour sizes themselves"""
    import smooth_cov_ref as SV
    import smooth_ref as SR
    _, _, kind, args, kw = run
    kind = kind[len("sized_"):] if kind.startswith("sized_") else kind
    kw = dict(kw)
    times = kw.pop("times", None)
    sig, iters = args[-2:]
    a = args[:-2]
    if kind in ("cam", "rig"):
        out, res, trace = (SR.smooth if kind == "cam" else SR.smooth_rig)(*a, *sig, iters, times=times, **kw)
        return out, res, None, trace
    if kind in ("cam_seq", "rig_seq"):
        return (SR.smooth_sequences if kind == "cam_seq" else SR.smooth_rig_sequences)(*a, *sig, iters, times=times, **kw) + (None, None)
    if kind == "cam_cov":
        out, res, _ = SR.smooth(*a, *sig, iters, times=times, **kw)
        return out, res, SV.smooth_cov(*a[:5], out, res, *sig, times=times, **kw)[0], None
    assert kind == "rig_cov", kind
    out, res, _ = SR.smooth_rig(*a, *sig, iters, times=times, **kw)
    return out, res, SV.smooth_rig_cov(*a[:4], out, res, *sig, times=times, **kw)[0], None


def fields(out):
    """{field of FIELDS: its values, flat} of a run's four outputs, and the run's dims"""
    poses, res, cov, trace = out
    res = np.atleast_1d(res)
    f = {"poses." + k: poses[k] for k in POSE_F8 + POSE_I4}
    f.update({"res." + k: res[k] for k in RES_F8 + RES_I4})
    if cov is not None:
        assert len(cov) == len(poses) and np.array_equal(cov["cov"], np.swapaxes(cov["cov"], 1, 2))
        f.update({"cov.cov": cov["cov"][:, TRIL[0], TRIL[1]], "cov.sigma_px": cov["sigma_px"], "cov.dof": cov["dof"], "cov.status": cov["status"]})
    n_posed = n_trials = n_choice = 0
    if trace is not None:
        n_posed, n_trials, n_choice = len(trace["posed"]), len(trace["lins"]), len(trace["choice"])
        assert n_choice in (0, n_posed) and trace["d"].shape == (n_posed, 2) and trace["tr"].shape == (n_posed, 2, 2)
        f.update({"trace.posed": np.asarray(trace["posed"], dtype=np.int64), "trace.choice": trace["choice"], "trace.d": trace["d"], "trace.tr": trace["tr"],
                  "trace.cost": np.array([lin["cost"] for _, lin in trace["lins"]], dtype=np.float64)})
    out = {}
    for name, dbl, _ in FIELDS:
        a = np.asarray(f.get(name, ()))
        out[name] = np.ascontiguousarray(a, dtype=np.float64).ravel() if dbl else a.astype(np.int32).ravel()
        assert dbl or np.array_equal(out[name], a.ravel())
    return out, (len(poses), len(res), int(cov is not None), int(trace is not None), n_posed, n_trials, n_choice)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def third_row(bits):
    """the bit patterns (n x 16 int64, flat) of a prediction of the T whose bit patterns are given, from entries the prediction
    leaves alone: the third row of the rotation as the cross product of the first two, 0 everywhere else.  A plain run's T is
    stored as its difference from this, which leaves a few last bits of three of its twelve free entries"""
    T = bits.view(np.float64).reshape(-1, 16)
    a, b = T[:, 0:3], T[:, 4:7]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    out = np.zeros(T.shape)
    out[:, 8:11] = np.where(np.isfinite(c), c, 0.0)
    return out.view(np.int64).ravel()


def pack(recorded):
    """recorded: [(run, outputs)] in runs() order -> the arrays of the file"""
    keys, dims, delta = [], [], []
    streams = {n: [] for n, _, _ in FIELDS}
    prev = None
    for run, out in recorded:
        cur, dm = fields(out)
        rev = bool(run[4].get("reverse"))
        row = []
        for n, dbl, _ in FIELDS:
            if not dbl:
                streams[n].append(cur[n])
                continue
            d = int(rev and prev is not None and len(prev[n]) == len(cur[n]) and len(cur[n]) > 0)
            row.append(d)
            base = _bits(prev[n]) if d else third_row(_bits(cur[n])) if n == "poses.T" else 0
            streams[n].append(_bits(cur[n]) - base)
        prev = None if rev else cur
        keys.append(run[0])
        dims.append(dm)
        delta.append(row)
    arrays = dict(keys=np.array(keys), dims=np.array(dims, dtype=np.int32), delta=np.array(delta, dtype=np.int8), layout=np.array(LAYOUT))
    for n, dbl, _ in FIELDS:
        if dbl:
            arrays[n] = np.ascontiguousarray(np.concatenate(streams[n]).astype(np.int64).view(np.uint8).reshape(-1, 8).T)     # byte planes, (8, n)
        else:
            arrays[n] = np.concatenate(streams[n]).astype(np.int32)
    return arrays


def save(path, arrays):
    """an .npz (np.load reads it) whose members are LZMA-compressed"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as zf:
        for k, a in arrays.items():
            with zf.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def counts(dm, per):
    n_frames, n_res, has_cov, _, n_posed, n_trials, n_choice = dm
    return per[0] * n_frames + per[1] * n_res + per[2] * n_frames * has_cov + per[3] * n_posed + per[4] * n_trials


def load(path=OUT):
    """{key: (dims, {field: values, flat})} with every double as it was recorded"""
    z = dict(np.load(path))
    out, at, prev = {}, {n: 0 for n, _, _ in FIELDS}, None
    col = {n: i for i, n in enumerate(n for n, dbl, _ in FIELDS if dbl)}
    for n in col:
        z[n] = np.ascontiguousarray(z[n].T).view(np.int64).ravel()
    for i, key in enumerate(z["keys"]):
        dm = tuple(int(x) for x in z["dims"][i])
        e = {}
        for n, dbl, per in FIELDS:
            cnt = counts(dm, per)
            if n == "trace.choice":
                cnt = dm[6]
            a = z[n][at[n]:at[n] + cnt].copy()
            at[n] += cnt
            if dbl:
                if z["delta"][i][col[n]]:
                    a += prev[n].view(np.int64)
                elif n == "poses.T":
                    a += third_row(a)
                a = a.view(np.float64)
            e[n] = a
        out[str(key)] = (dm, e)
        prev = e
    assert all(at[n] == len(z[n]) for n, _, _ in FIELDS)
    return out


def rel(a, b):
    """0 if the bytes are equal; else the largest |a - b| / |b| over the entries (where the record b is 0, a must be 0)"""
    if a.tobytes() == b.tobytes():
        return 0.0
    assert a.shape == b.shape and np.array_equal(a[b == 0], b[b == 0]) and np.array_equal(np.isfinite(a), np.isfinite(b))
    nz = (b != 0) & np.isfinite(b)
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


def compare(key, e, out):
    """a run's outputs against its record e.  Asserts what must be equal in any case: the dims (frames, result records, posed
    frames, trials) and every integer field -- the counts, the statuses, seed_slot, n_rejected, posed, choice.  Returns the
    largest relative difference of the doubles, 0.0 where their bytes are the recorded ones, and the field it is at."""
    cur, dm = fields(out)
    assert dm == e[0], (key, dm, e[0])
    worst = (0.0, "")
    for n, dbl, _ in FIELDS:
        if dbl:
            worst = max(worst, (rel(cur[n], e[1][n]), n))
        else:
            assert np.array_equal(cur[n], e[1][n]), (key, n, cur[n], e[1][n])
    return worst


def main(argv):
    if argv[:1] == ["record"] and len(argv) == 2:
        parent = os.path.abspath(argv[1])
        sys.path[:0] = [parent, os.path.dirname(parent)]
        recorded = []
        for run in runs():
            recorded.append((run, run_parent(run)))
            print(run[0], flush=True)
        save(OUT, pack(recorded))
        back = load()
        assert list(back) == [r[0][0] for r in recorded]
        for run, out in recorded:
            assert compare(run[0], back[run[0]], out)[0] == 0.0, run[0]
        print("%d runs, %d bytes" % (len(recorded), os.path.getsize(OUT)))
    elif argv == ["compare"]:
        sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
        rec = load()
        todo = runs()
        assert [r[0] for r in todo] == list(rec)
        for name in SETS:
            worst = (0.0, "", "")
            for run in [r for r in todo if r[1] == name]:
                worst = max(worst, compare(run[0], rec[run[0]], run_one(run)) + (run[0],))
            print("%s: largest relative difference %.3g%s over %d runs" % (name, worst[0], " (%s of %s)" % worst[1:] if worst[0] else "",
                                                                           sum(r[1] == name for r in todo)), flush=True)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
