"""The de-duplication stage (S8) as a plain statement, for the tests of csrc/k_dedup.inc and of asl_debug_dedup.

One frame: upstream's loop over the records in the order of decoding (ascending cluster key).  Every pair of records
with the same id whose quads overlap loses one member: the worse by lower hamming, then higher margin, then the eight
corner coordinates in order (the smaller wins); of two equal records the later one stays.  The survivors are sorted by
(id, hamming, corners).  Arithmetic in float64 (the margin is a float32), one operation at a time as the C oracle and the
kernel do it with contraction off, so the three agree bit for bit and no test needs a tolerance.

The overlap of one record with all its later candidates is evaluated as NumPy arrays -- the same float64 operations,
element by element -- because a group of 1024 records of one id that do not overlap is 524,000 tests.

Records are 96-byte structured arrays with the fields of asl_detection (_lib.DET_DTYPE)."""
import numpy as np

DEDUP_MAX = 1024   # records of one frame the device sorts; a frame above it comes back empty and is counted
KEY_MASK = (1 << 48) - 1


def _cross(a, b, p):
    """(b - a) x (p - a); a, b, p: (..., 2)"""
    return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])


def _point_in_quad(q, p):
    """q (..., 4, 2), p (..., 2): no side of q has p strictly on its left, or none strictly on its right"""
    c = _cross(q, np.roll(q, -1, axis=-2), p[..., None, :])
    return ((c > 0).sum(axis=-1) == 0) | ((c < 0).sum(axis=-1) == 0)


def quads_overlap(a, b):
    """a (4, 2) against b (m, 4, 2) -> (m,) bool: two sides cross, or corner 0 of one lies in the other"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 4, 2)
    a0, a1 = a[None, :, None, :], np.roll(a, -1, axis=0)[None, :, None, :]   # side i of a: (1, 4, 1, 2)
    b0, b1 = b[:, None, :, :], np.roll(b, -1, axis=1)[:, None, :, :]         # side j of b: (m, 1, 4, 2)
    d1, d2 = _cross(a0, a1, b0), _cross(a0, a1, b1)
    d3, d4 = _cross(b0, b1, a0), _cross(b0, b1, a1)
    crossing = (((d1 > 0) != (d2 > 0)) & ((d3 > 0) != (d4 > 0))).any(axis=(1, 2))
    return crossing | _point_in_quad(a[None], b[:, 0]) | _point_in_quad(b, a[None, 0])


def prefer(a, b):
    """< 0: a stays, otherwise b"""
    if a["hamming"] != b["hamming"]:
        return -1 if a["hamming"] < b["hamming"] else 1
    if a["margin"] != b["margin"]:
        return -1 if a["margin"] > b["margin"] else 1
    for x, y in zip(a["corners"].ravel().tolist(), b["corners"].ravel().tolist()):
        if x != y:
            return -1 if x < y else 1
    return 0


def eliminate(d):
    """d: one frame's records in the order of decoding -> (n,) bool, the records upstream's loop keeps"""
    n = len(d)
    alive = np.ones(n, dtype=bool)
    ids, corners = d["id"], d["corners"]
    for i0 in range(n):
        if not alive[i0]:
            continue
        cand = i0 + 1 + np.nonzero((ids[i0 + 1:] == ids[i0]) & alive[i0 + 1:])[0]
        if len(cand) == 0:
            continue
        for i1 in cand[quads_overlap(corners[i0], corners[cand])]:
            if prefer(d[i0], d[i1]) < 0:
                alive[i1] = False
            else:
                alive[i0] = False
                break
    return alive


def dedup_frame(recs, keys):
    """One frame's records and their cluster keys -> the survivors, sorted by (id, hamming, corners)."""
    recs = np.asarray(recs)
    keys = np.asarray(keys, dtype=np.uint64) & np.uint64(KEY_MASK)
    d = recs[np.argsort(keys, kind="stable")]
    d = d[eliminate(d)]
    order = sorted(range(len(d)), key=lambda i: (int(d["id"][i]), int(d["hamming"][i])) + tuple(d["corners"][i].ravel().tolist()))
    return d[order]


def dedup(recs, keys, n_frames, cap_per_frame=DEDUP_MAX):
    """What asl_debug_dedup returns for these records: (survivors frame by frame, (n_frames,) int32 counts,
    [survivors, overflow, frames above DEDUP_MAX]).  A frame with more records than cap_per_frame overflows: every frame
    comes back empty and the overflow counter is positive (returned as 1: how many records find the list full before the
    launch backs out is not defined)."""
    recs = np.asarray(recs)
    keys = np.asarray(keys, dtype=np.uint64)
    npf = np.zeros(n_frames, dtype=np.int32)
    per_frame = np.bincount(recs["frame"], minlength=n_frames)
    if (per_frame > cap_per_frame).any():
        return recs[:0].copy(), npf, np.array([0, 1, 0], dtype=np.int64)
    out, limit = [], 0
    for f in np.nonzero(per_frame)[0]:
        if per_frame[f] > DEDUP_MAX:
            limit += 1
            continue
        m = recs["frame"] == f
        kept = dedup_frame(recs[m], keys[m])
        npf[f] = len(kept)
        out.append(kept)
    out = np.concatenate(out) if out else recs[:0].copy()
    return out, npf, np.array([len(out), 0, limit], dtype=np.int64)
