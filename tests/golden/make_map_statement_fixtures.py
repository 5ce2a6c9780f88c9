#!/usr/bin/env python3
"""Record tests/golden/map_statements.npz: what the four NumPy statements of the tag-map reconstruction (tests/map_ref.py
and its robust, rig and sized copies, tests/map_<robust|rig|sized>_ref.py) returned before they became the one statement
tests/map_ref.py.

Recorded at commit 0450cc604d76449338901a44890380ff8e3e0aa4 ("Test decimation, threshold and labelling at their tile and
word edges"), the last one that has the four.  The recorder imports everything (cases, statements, package) from a checkout
of that commit and runs on the CPU only:

    git worktree add --detach /tmp/parent 0450cc6
    python tests/golden/make_map_statement_fixtures.py record /tmp/parent/tests     # writes map_statements.npz
    python tests/golden/make_map_statement_fixtures.py compare                      # the one statement against the record

runs() is the list of recorded calls, built from the cases modules on sys.path; tests/test_map_statement_golden.py runs the
same list through the one statement and compare() states what must be equal and what is measured.  Every run is recorded by
the statement that owned its case: map_cases.cpu_cases() and solver_edge_cases.map_cases() by map_ref (the cpu cases at
HUBER by the robust copy), map_robust_cases.compared_cases() by the robust copy, map_rig_cases' main, edge and compared
cases by the rig copy, map_sized_cases' by the sized copy; each at the huber_px and max_iters its tests use (a tail case
also at the full trial count), plain and with reverse=True where the statement has it.

The file (the key list "layout" says the same): the runs' outputs laid end to end.  The map and tag_std are stored at the
valid ids only (the recorder asserts that every other row is zero).  A slot_weight that is all 0 and 1 is stored as its bits;
map_ref.map_frames returned none ("weight_kind" 0: the one statement's must be 0 and 1 with n_obs ones at status 0).  The
doubles of a reverse=True run are stored as the int64 difference of their bit patterns from the plain run before it, which
is a few last bits and so compresses, and all doubles as eight byte planes; load() undoes both, so every double is the
recorded one exactly.
"""
import importlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "map_statements.npz")
LAYOUT = ("keys", "shape (n_ids, n_cams, n_frames, max_tags)", "delta (1: doubles are int64 differences from the run before)",
          "res", "n_valid", "valid_ids", "map_T", "map_size", "tag_std", "poses", "pose_f8",
          "weight_kind (0: none returned, 1: bits, 2: doubles)", "weight_bits", "weight_f8", "layout")
LOOSE_RES = ("cost_seed", "cost", "rms_px", "rms_seed_px")
INT_RES = ("n_frames_used", "n_tags", "n_obs", "n_obs_dropped", "iterations", "world_id", "status", "n_soft")
INT_POSE = ("n_tags", "n_rejected", "status", "seed_slot")


def runs():
    """(key, set name, statement, args, kwargs) of every recorded call.  statement "camera": args (obs (F, S), n_ids, K, dist,
    tag_size); "rig": args (obs (C, F, S), n_ids, rig, tag_size, tag_sizes).  A reverse=True run follows its plain run."""
    import localize_cases as LC
    import map_cases as MC
    import map_rig_cases as GC
    import map_robust_cases as RBC
    import map_sized_cases as ZC
    import solver_edge_cases as E

    def both(key, name, st, args, kw):
        return [(key + "/fwd", name, st, args, kw), (key + "/rev", name, st, args, dict(kw, reverse=True))]

    out = []
    # map
    K = MC.K_bench()
    for n, obs, dist, w in MC.cpu_cases(K):
        out.append(("map/%s" % n, "map", "camera", (obs, MC.N_IDS, K, dist, LC.TAG_INNER), dict(world_id=w)))
        out.append(("map/%s/h%g" % (n, RBC.HUBER), "map", "camera", (obs, MC.N_IDS, K, dist, LC.TAG_INNER), dict(world_id=w, huber_px=RBC.HUBER)))
    # robust
    for n, obs, dist, iters in RBC.compared_cases():
        for it in sorted({iters, RBC.ITERS}):
            for hub in (0.0, RBC.HUBER):
                out += both("robust/%s/h%g/i%d" % (n, hub, it), "robust", "camera", (obs, MC.N_IDS, RBC.K, dist, LC.TAG_INNER), dict(huber_px=hub, max_iters=it))
    # rig
    cases = dict(GC.main_cases(), **GC.edge_cases())
    compared = GC.compared_cases()
    assert {c[0] for c in compared} == set(cases)
    for n, obs, rig, hub, iters in compared:
        for it in sorted({iters, GC.ITERS}):
            out += both("rig/%s/h%g/i%d" % (n, hub, it), "rig", "rig", (obs, GC.N_IDS, rig, GC.TAG, None), dict(huber_px=hub, max_iters=it))
    # sized
    cases = dict(ZC.main_cases(), **ZC.edge_cases())
    compared = ZC.compared_cases()
    assert {c[0] for c in compared} == set(cases)
    for n, obs, rig, t, hub, iters in compared:
        for it in sorted({iters, ZC.ITERS}):
            out += both("sized/%s/h%g/i%d" % (n, hub, it), "sized", "rig", (obs, ZC.N_IDS, rig, ZC.TAG, t), dict(huber_px=hub, max_iters=it))
    # edges
    for n, obs, n_ids, dist, w, kw, _ in E.map_cases():
        out.append(("edges/%s" % n, "edges", "camera", (obs, n_ids, E.K, dist, LC.TAG_INNER), dict(kw, world_id=w)))
    return out


SETS = ("map", "robust", "rig", "sized", "edges")


def run_parent(run):
    """the call through the statement that owned it at the recorded commit: its four or five outputs"""
    _, name, st, args, kw = run
    if name in ("map", "edges"):
        name = "robust" if "huber_px" in kw else ""
    statement = importlib.import_module("map_%s_ref" % name if name else "map_ref")
    if name == "rig":
        return statement.map_frames(*args[:4], **kw)              # no size table
    return statement.map_frames(*args, **kw)


def run_one(run):
    """the call through the one statement: five outputs"""
    import map_ref
    _, _, st, args, kw = run
    return (map_ref.map_frames if st == "camera" else map_ref.map_rig_frames)(*args, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def pose_doubles(poses):
    """(F, 18): T, rms_px, rms_seed_px"""
    return np.concatenate([poses["T"].reshape(len(poses), 16), poses["rms_px"][:, None], poses["rms_seed_px"][:, None]], axis=1)


def pack(recorded):
    """recorded: [(run, outputs)] in runs() order -> the arrays of the file"""
    keys, shape, delta, res, n_valid, ids, wkind, wbits = [], [], [], [], [], [], [], []
    f8 = {"map_T": [], "tag_std": [], "pose_f8": [], "weight_f8": []}
    size, poses = [], []
    prev = None
    for run, out in recorded:
        key, _, st, args, kw = run
        obs = np.asarray(args[0])
        C, F, S = obs.shape if st == "rig" else (1,) + obs.shape
        r, tmap, std, po = out[:4]
        v = np.flatnonzero(tmap["valid"])
        rest = np.setdiff1d(np.arange(len(tmap)), v)
        assert not tmap["T"][rest].any() and not tmap["size"][rest].any() and not std[rest].any() and set(np.unique(tmap["valid"])) <= {0, 1}
        cur = {"map_T": tmap["T"][v], "tag_std": std[v], "pose_f8": pose_doubles(po)}
        if len(out) == 4:
            wkind.append(0)
        else:
            w = np.asarray(out[4]).reshape(C, F, S)
            if np.isin(w, (0.0, 1.0)).all():
                wkind.append(1)
                wbits.append(np.packbits(w.ravel() == 1.0))
            else:
                wkind.append(2)
                cur["weight_f8"] = w.ravel()
        d = int(bool(kw.get("reverse")) and prev is not None and prev.keys() == cur.keys() and all(prev[k].shape == cur[k].shape for k in cur))
        for k, a in cur.items():
            f8[k].append((_bits(a) - _bits(prev[k]) if d else _bits(a)).ravel())
        prev = None if kw.get("reverse") else cur
        keys.append(key)
        shape.append((len(tmap), C, F, S))
        delta.append(d)
        res.append(r)
        n_valid.append(len(v))
        ids.append(v.astype(np.int32))
        size.append(tmap["size"][v])
        ints = np.zeros(F, dtype=[(k, "<i4") for k in INT_POSE])
        for k in INT_POSE:
            ints[k] = po[k]
        poses.append(ints)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)   # noqa: E731
    arrays = dict(keys=np.array(keys), shape=np.array(shape, dtype=np.int32), delta=np.array(delta, dtype=np.int8), res=np.array(res),
                  n_valid=np.array(n_valid, dtype=np.int32), valid_ids=cat(ids, np.int32), map_size=cat(size, np.float32),
                  poses=np.concatenate(poses), weight_kind=np.array(wkind, dtype=np.int8), weight_bits=cat(wbits, np.uint8),
                  layout=np.array(LAYOUT))
    for k, xs in f8.items():
        arrays[k] = np.ascontiguousarray(cat(xs, np.int64).view(np.uint8).reshape(-1, 8).T)      # byte planes, (8, n)
    return arrays


def save(path, arrays):
    """an .npz (np.load reads it) whose members are LZMA-compressed: a fifth smaller than np.savez_compressed's"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as zf:
        for k, a in arrays.items():
            with zf.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def load(path=OUT):
    """{key: dict(shape, res, valid_ids, map_T (n, 12), map_size, tag_std (n, 6), pose_ints, pose_f8 (F, 18), weight (C, F, S) or
    None)} with every double as it was recorded"""
    z = dict(np.load(path))
    for k in ("map_T", "tag_std", "pose_f8", "weight_f8"):
        z[k] = np.ascontiguousarray(z[k].T).view(np.int64).ravel()
    out = {}
    at = dict(v=0, p=0, wb=0, wf=0, T=0, std=0, pf=0)
    prev = None
    for i, key in enumerate(z["keys"]):
        n_ids, C, F, S = (int(x) for x in z["shape"][i])
        nv, kind, d = int(z["n_valid"][i]), int(z["weight_kind"][i]), int(z["delta"][i])

        def take(name, cursor, n, sh, was):
            a = z[name][at[cursor]:at[cursor] + n].copy()
            at[cursor] += n
            if d:
                a += was.view(np.int64).ravel()
            return a.view(np.float64).reshape(sh)
        e = dict(shape=(n_ids, C, F, S), res=z["res"][i], valid_ids=z["valid_ids"][at["v"]:at["v"] + nv], map_size=z["map_size"][at["v"]:at["v"] + nv],
                 pose_ints=z["poses"][at["p"]:at["p"] + F])
        e["map_T"] = take("map_T", "T", 12 * nv, (nv, 12), prev and prev["map_T"])
        e["tag_std"] = take("tag_std", "std", 6 * nv, (nv, 6), prev and prev["tag_std"])
        e["pose_f8"] = take("pose_f8", "pf", 18 * F, (F, 18), prev and prev["pose_f8"])
        at["v"] += nv
        at["p"] += F
        n = C * F * S
        if kind == 0:
            e["weight"] = None
        elif kind == 1:
            nb = (n + 7) // 8
            e["weight"] = np.unpackbits(z["weight_bits"][at["wb"]:at["wb"] + nb])[:n].astype(np.float64).reshape(C, F, S)
            at["wb"] += nb
        else:
            e["weight"] = take("weight_f8", "wf", n, (C, F, S), prev and prev["weight"])
        out[str(key)] = e
        prev = e
    assert at["T"] == len(z["map_T"]) and at["wf"] == len(z["weight_f8"]) and at["wb"] == len(z["weight_bits"]) and at["p"] == len(z["poses"])
    return out


def rel(a, b):
    """largest |a - b| / |b| over the entries; where the record b is 0, a must be 0"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape and np.array_equal(a[b == 0], b[b == 0])
    nz = b != 0
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


def compare(key, e, out):
    """a run's five outputs against its record e.  Asserts what must be equal: every integer field of the result and of the
    poses, valid, size, the map's T, the poses' T and slot_weight byte for byte.  Returns the largest relative difference of
    the remaining doubles (cost, cost_seed, the result's rms, the per-frame rms, tag_std) and the field it is at."""
    r, tmap, std, po, w = out
    n_ids, C, F, S = e["shape"]
    assert len(tmap) == n_ids and len(po) == F and std.shape == (n_ids, 6) and w.shape in ((C, F, S), (F, S)), key
    for k in INT_RES:
        assert r[k] == e["res"][k], (key, k, r[k], e["res"][k])
    for k in INT_POSE:
        assert np.array_equal(po[k], e["pose_ints"][k]), (key, k)
    v = np.flatnonzero(tmap["valid"])
    rest = np.setdiff1d(np.arange(n_ids), v)
    assert np.array_equal(v, e["valid_ids"]) and set(np.unique(tmap["valid"])) <= {0, 1}, key
    assert not tmap["T"][rest].any() and not tmap["size"][rest].any() and not std[rest].any(), key
    assert tmap["size"][v].tobytes() == e["map_size"].tobytes(), key
    assert np.ascontiguousarray(tmap["T"][v]).tobytes() == e["map_T"].tobytes(), (key, "map T")
    assert np.ascontiguousarray(po["T"]).tobytes() == np.ascontiguousarray(e["pose_f8"][:, :16]).tobytes(), (key, "pose T")
    if e["weight"] is None:
        assert np.isin(w, (0.0, 1.0)).all() and w.sum() == (r["n_obs"] if r["status"] == 0 else 0), key
    else:
        assert np.asarray(w, dtype=np.float64).tobytes() == e["weight"].tobytes(), (key, "slot_weight")
    worst = max((rel(r[k], e["res"][k]), k) for k in LOOSE_RES)
    worst = max(worst, (rel(po["rms_px"], e["pose_f8"][:, 16]), "poses.rms_px"), (rel(po["rms_seed_px"], e["pose_f8"][:, 17]), "poses.rms_seed_px"),
                (rel(std[v], e["tag_std"]), "tag_std"))
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
        print("%d runs, %d bytes" % (len(recorded), os.path.getsize(OUT)))
    elif argv == ["compare"]:
        sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
        rec = load()
        todo = runs()
        assert [r[0] for r in todo] == list(rec)
        worst = (0.0, "", "")
        for run in todo:
            worst = max(worst, compare(run[0], rec[run[0]], run_one(run)) + (run[0],))
        print("largest relative difference %.3g (%s of %s) over %d runs" % (worst + (len(todo),)))
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
