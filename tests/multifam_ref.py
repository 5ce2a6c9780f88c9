"""The statement of a detector of several families: upstream's loop over its family list, composed from the CPU oracle's
stage functions (oracle_lib) plus aso_decode_quad.  TEST INFRASTRUCTURE ONLY.

Per frame: decimate, threshold, label components, gather gradient clusters; for each border polarity some family has,
fit quads with a stand-in family (the fit reads only width_at_border and reversed_border of its family: the stand-in's
width_at_border is the minimum tag width, min over the families of max(3, width_at_border / decimate), times decimate);
order the quads by cluster; rescale the corners to the full image as the oracle's own detector does; refine the edges;
decode every quad against every family in table order (aso_decode_quad refuses a family of the other polarity), adding
id_base; de-duplicate and sort."""
import ctypes as C
import types

import numpy as np

import oracle_lib as O
from aprilslam_amd import _lib


def min_tag_width(fams, decimate):
    return min(max(3, f.width_at_border // decimate) for f in fams)


def quads(dec, pts, fams, decimate):
    """the quads of every wanted polarity, by cluster"""
    out = []
    for rev in sorted({bool(f.reversed_border) for f in fams}):
        f0 = fams[0]
        stand_in = types.SimpleNamespace(nbits=f0.nbits, width_at_border=min_tag_width(fams, decimate) * decimate, total_width=f0.total_width,
                                         reversed_border=rev, codes=f0.codes, bit_x=f0.bit_x, bit_y=f0.bit_y)
        out += O.fit_quads(dec, pts, stand_in, decimate)
    return sorted(out, key=lambda q: q["cluster"])


def decode_quad(gray, fam_c, maxhamming, p, reversed_border):
    """aso_decode_quad on corners p (4, 2) in full-resolution pixels: a dict like oracle_lib's, or None"""
    h, w = gray.shape
    q = O.AsoQuad()
    for i in range(4):
        q.p[i][0], q.p[i][1] = float(p[i][0]), float(p[i][1])
    q.reversed_border = int(reversed_border)
    det = O.AsoDetection()
    if not O.lib().aso_decode_quad(gray.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, w, C.byref(fam_c.c), int(maxhamming), C.byref(q), C.byref(det)):
        return None
    return det


def detect(gray, fams, id_base, decimate=2, maxhamming=1):
    """[dict(id, hamming, margin, center, corners)] of one gray frame, in the detector's output order; id is global"""
    gray = np.ascontiguousarray(gray, dtype=np.uint8)
    dec = O.decimate(gray, decimate)
    th = O.threshold(dec)
    lab, sz = O.connected_components(th)
    pts = O.gradient_clusters(th, lab, sz)
    tables = [O.Family(f) for f in fams]
    recs = []
    for q in quads(dec, pts, fams, decimate):
        p = (q["p"] - 0.5) * decimate + 0.5 if decimate > 1 else q["p"]
        p = O.refine_edges(gray, p, q["reversed_border"], decimate)
        for t, base in zip(tables, id_base):
            det = decode_quad(gray, t, maxhamming, p, q["reversed_border"])
            if det is not None:
                recs.append((det.id + int(base), det.hamming, det.margin, 0, tuple(det.center), tuple(tuple(c) for c in det.corners)))
    kept = O.dedup_and_sort(np.array(recs, dtype=_lib.DET_DTYPE)) if recs else []
    return tuple(dict(id=int(d["id"]), hamming=int(d["hamming"]), margin=float(d["margin"]), center=np.array(d["center"]),
                      corners=np.array(d["corners"])) for d in kept)


def merged_single_runs(gray, fams, id_base, decimate=2, maxhamming=1):
    """One single-family oracle run per family, ids moved to the global range, merged in (id) order: what `detect` must
    equal wherever no quad decodes in two families and the families' minimum tag widths let the same clusters through."""
    out = []
    for f, base in zip(fams, id_base):
        for d in O.detect_gray(gray, f, decimate, maxhamming=maxhamming):
            out.append(dict(d, id=d["id"] + int(base)))
    return tuple(sorted(out, key=lambda d: d["id"]))
