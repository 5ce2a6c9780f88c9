"""NumPy statement of the tag-map reconstruction for tags of different known sizes (asl_map_sized_* / asl_map_rig_sized_*,
aprilslam_amd/csrc/k_map.inc): map_rig_ref.map_frames with a half side per tag and the records' PnP poses scaled.  Test
infrastructure; what is not named here is map_rig_ref's.

The rule (map_tag_half, sized_ref.py) on the caller's table tag_sizes, (n_ids,) float32:

  0                    the tag has the call's tag_size: half = float32(tag_size / 2), as in map_rig_ref
  > 0, finite          the tag's own side: h_id = float32(size) * float32(0.5)
  negative, not finite ValueError naming the id (the device: ASL_EINVAL, nothing written)

and where it enters:

  corners  every pass that forms a tag's corners (+-h, +-h, 0) uses that tag's h: the sweeps' costs, the flip test's tag_lm,
           the behind test, the LM's blocks and costs, the robust terms and the seed and final per-view costs.  A tag's LM
           has one h, so map_rig_ref.tag_lm serves as it is.  corner_terms and view_blocks work row by row; given the views'
           halves they run map_rig_ref's function once per distinct half over that half's views, in view order, and put the
           rows back where they were.  With one half among the views that is map_rig_ref's own call.
  seeds    a record's PnP pose T was solved at tag_size; a sized tag's translation is multiplied by k = h_id / half before
           T proposes anything (the chain's frame and tag halves, the sweeps' candidates plain and mirrored: the mirrored
           minimum is formed from the scaled pose).  A tag without a size keeps T as it is.  The flip test's mirror comes
           from the map pose.
  output   map["size"] = the table's entry for every mapped id.

With an all-zero table (or None) every call below is map_rig_ref's with the same arguments in the same order, so the results
are map_rig_ref.map_frames' byte for byte (tests/test_map_sized_ref.py).

trace receives, beyond map_rig_ref's entries: "ids"; "chain_frames" [(frame, id of the seeding view)] and "chain_tags" [id
the chain placed]; "sweep_mirrored" [("frame", frame, id) or ("tag", id, id): the winning candidate was the mirrored pose of a
view of that id]; "behind" [id of every view the behind test dropped].
"""
import numpy as np
from scipy.linalg import solve_triangular

import localize_ref as LR
import map_rig_ref as GR
import rig_ref
from aprilslam_amd._lib import CAM_POSE_DTYPE, MAP_RESULT_DTYPE, MAP_TAG_DTYPE
from map_ref import BEHIND_MARGIN, MAX_CAND, MAX_MAP_TAGS, SWEEPS, gn_oracle, inv, mirror4, obj3, rec4
from map_rig_ref import assemble, fold_pairs, margin, mountings, tag_lm


def size_table(tag_sizes, n_ids):
    """(n_ids,) float32; None: all zero.  A negative or non-finite entry is refused"""
    if tag_sizes is None:
        return np.zeros(n_ids, dtype=np.float32)
    t = np.asarray(tag_sizes, dtype=np.float32)
    if t.shape != (n_ids,):
        raise ValueError("tag_sizes must hold n_ids = %d entries" % n_ids)
    bad = np.flatnonzero(~(np.isfinite(t) & (t >= 0)))
    if len(bad):
        raise ValueError("tag_sizes[%d] must be 0 or positive and finite" % bad[0])
    return t


def tag_half(size, half):
    """sized_ref.tag_half on a table entry"""
    return float(np.float32(size) * np.float32(0.5)) if size > 0 else half


def scaled(T, size, h, half):
    """a record's camera<-tag (4x4) as it is for a tag of half side h: sized_ref.tag_pose"""
    if size > 0:
        T[:3, 3] = T[:3, 3] * (h / half)
    return T


def by_half(fn, hv, n_out):
    """fn(rows, h) -> n_out arrays with one row per view, run once per distinct half of hv (n,) over its views (rows: their
    indices, ascending) and put back in place.  One half: fn's own result"""
    hv = np.asarray(hv, dtype=np.float64)
    halves = np.unique(hv)
    if len(halves) <= 1:
        return fn(np.arange(len(hv)), float(halves[0]) if len(halves) else 0.0)
    out = None
    for h in halves:
        rows = np.flatnonzero(hv == h)
        got = fn(rows, float(h))
        if out is None:
            out = [np.zeros((len(hv),) + g.shape[1:], dtype=g.dtype) for g in got]
        for o, g in zip(out, got):
            o[rows] = g
    return tuple(out)


def corner_terms(table, vc, Wv, G, uv, hv, k):
    """map_rig_ref.corner_terms with the views' own halves hv (n,)"""
    return by_half(lambda r, h: GR.corner_terms(table, vc[r], Wv[r], G[r], uv[r], h, k), hv, 5)


def view_costs(table, vc, Wv, G, uv, hv, k=0.0):
    """(n,) cost of each view"""
    return corner_terms(table, np.asarray(vc), Wv, G, uv, hv, k)[0].sum(axis=1)


def view_blocks(table, W, G, oc, ot, ovc, uv, hv, k=0.0, trace=None):
    """map_rig_ref.view_blocks with the views' own halves hv (M,)"""
    return by_half(lambda r, h: GR.view_blocks(table, W, G, oc[r], ot[r], ovc[r], uv[r], h, k, trace), hv, 2)


def joint_linearise(table, W, G, oc, ot, ovc, uv, hv, cam_col, tag_col, n_par, k=0.0, trace=None, fold=True):
    """map_rig_ref.joint_linearise over view_blocks above"""
    cost_v, B = view_blocks(table, W, G, oc, ot, ovc, uv, hv, k, trace)
    if fold:
        B, heads = fold_pairs(B, oc, ot)
        oc, ot = oc[heads], ot[heads]
        if trace is not None:
            trace["views"], trace["pairs"] = len(cost_v), len(heads)
    H, g = assemble(B, oc, ot, cam_col, tag_col, n_par)
    return float(cost_v.sum()), H, g


def won(trace, what, key, costs, src):
    """note a sweep whose winning candidate is a mirrored one: candidates 1, 2 / 3, 4 / ... are view k's plain and mirrored"""
    best = int(np.argmin(costs))
    if trace is not None and best > 0 and best % 2 == 0:
        trace["sweep_mirrored"].append((what, key, src[(best - 1) // 2]))


def map_frames(obs, n_ids, rig, tag_size, tag_sizes=None, world_id=-1, huber_px=0.0, max_iters=30, with_std=True, trace=None, reverse=False):
    """(result MAP_RESULT_DTYPE record, map (n_ids,) MAP_TAG_DTYPE, tag_std (n_ids, 6), poses (n_frames,) CAM_POSE_DTYPE with
    T = world<-rig, slot_weight (n_cams, n_frames, max_tags)); tag_sizes: (n_ids,) sizes, 0 for tag_size, or None"""
    k = float(huber_px)
    if not (k >= 0 and np.isfinite(k)):
        raise ValueError("huber_px must be >= 0 and finite")
    obs = np.asarray(obs)
    C, F, S = obs.shape
    table = rig_ref.rig_table(rig)
    assert len(table) == C
    E = mountings(table)
    half = LR.half_size(tag_size)
    sizes = size_table(tag_sizes, n_ids)
    res = np.zeros((), dtype=MAP_RESULT_DTYPE)
    out_map = np.zeros(n_ids, dtype=MAP_TAG_DTYPE)
    tag_std = np.zeros((n_ids, 6))
    poses = np.zeros(F, dtype=CAM_POSE_DTYPE)
    poses["T"] = np.eye(4)
    poses["seed_slot"] = -1
    poses["status"] = 1
    slot_weight = np.zeros((C, F, S))

    # gather
    part = np.zeros((C, F, S), dtype=bool)
    for c in range(C):
        for f in range(F):
            seen = set()
            for s in range(S):
                i, fl = int(obs["id"][c, f, s]), int(obs["flags"][c, f, s])
                if (fl & 1) and 0 <= i < n_ids and i not in seen:
                    part[c, f, s] = True
                    seen.add(i)
    npart = part.sum(axis=(0, 2))
    ndist = [len({int(i) for i in obs["id"][:, f][part[:, f]]}) for f in range(F)]
    frames = [f for f in range(F) if ndist[f] >= 2]
    ids = sorted({int(i) for f in frames for i in obs["id"][:, f][part[:, f]]})
    tag_of = {i: j for j, i in enumerate(ids)}
    ob = [(n, tag_of[int(obs["id"][c, f, s])], f, c, s) for n, f in enumerate(frames) for c in range(C) for s in range(S) if part[c, f, s]]
    oc = np.array([o[0] for o in ob], dtype=np.int64)
    ot = np.array([o[1] for o in ob], dtype=np.int64)
    ofr = np.array([o[2] for o in ob], dtype=np.int64)
    ovc = np.array([o[3] for o in ob], dtype=np.int64)
    osl = np.array([o[4] for o in ob], dtype=np.int64)
    M, NC, NT = len(ob), len(frames), len(ids)
    if world_id < 0:
        world_id = ids[0] if ids else -1
    res["world_id"] = world_id
    res["n_obs_dropped"] = M
    if world_id not in tag_of:
        res["status"] = 1
        for f in frames:
            poses["status"][f] = 5
            poses["n_rejected"][f] = npart[f]
        return res, out_map, tag_std, poses, slot_weight
    if NT > MAX_MAP_TAGS:
        raise ValueError("more than %d tags" % MAX_MAP_TAGS)
    wt = tag_of[world_id]
    ht = np.array([tag_half(sizes[i], half) for i in ids])             # per tag: its half side
    hv = ht[ot]                                                        # per view
    rec = [obs[c, f, s] for c, f, s in zip(ovc, ofr, osl)]
    uv = np.stack([r["corners"].astype(np.float64).reshape(4, 2) for r in rec]) if M else np.zeros((0, 4, 2))
    To = [scaled(rec4(r["T"]), sizes[ids[j]], ht[j], half) for r, j in zip(rec, ot)]
    if trace is not None:
        trace.update(ids=ids, chain_frames=[], chain_tags=[], sweep_mirrored=[])
    seedable = np.array([bool(r["flags"] & 2) for r in rec], dtype=bool)
    area = np.array([LR.corner_area(r["corners"]) for r in rec])
    by_cam = [np.flatnonzero(oc == c) for c in range(NC)]
    by_tag = [np.flatnonzero(ot == j) for j in range(NT)]
    Ev, Evi = E[ovc] if M else np.zeros((0, 4, 4)), np.array([inv(E[c]) for c in ovc]) if M else np.zeros((0, 4, 4))

    def Wview(Wx, ms):
        """camera<-world of the views ms"""
        return Ev[ms] @ Wx[oc[ms]]

    # chain
    W = np.tile(np.eye(4), (NC, 1, 1))
    G = np.tile(np.eye(4), (NT, 1, 1))
    cplaced = np.zeros(NC, dtype=bool)
    tplaced = np.zeros(NT, dtype=bool)
    tplaced[wt] = True
    seed_slot = np.full(NC, -1)
    changed = True
    while changed:
        changed = False
        for c in range(NC):
            if cplaced[c]:
                continue
            cand = [m for m in by_cam[c] if seedable[m] and tplaced[ot[m]]]
            if cand:
                m = min(cand, key=lambda m: (-area[m], ot[m], ovc[m]))
                W[c] = Evi[m] @ (To[m] @ inv(G[ot[m]]))
                cplaced[c] = True
                seed_slot[c] = ovc[m] * S + osl[m]
                changed = True
                if trace is not None:
                    trace["chain_frames"].append((frames[c], ids[ot[m]]))
        for j in range(NT):
            if tplaced[j]:
                continue
            cand = [m for m in by_tag[j] if seedable[m] and cplaced[oc[m]]]
            if cand:
                m = min(cand, key=lambda m: (-area[m], m))
                G[j] = inv(Ev[m] @ W[oc[m]]) @ To[m]
                tplaced[j] = True
                changed = True
                if trace is not None:
                    trace["chain_tags"].append(ids[j])
    act = cplaced[oc] & tplaced[ot] if M else np.zeros(0, dtype=bool)

    # sweeps
    for _ in range(SWEEPS):
        Wn = W.copy()
        for c in range(NC):
            ms = [m for m in by_cam[c] if act[m]]
            if not cplaced[c] or not ms:
                continue
            cands, src = [W[c]], []
            sm = [m for m in ms if seedable[m]]
            for kk in LR.top_k([area[m] for m in sm], MAX_CAND):
                m = sm[kk]
                cands += [Evi[m] @ (To[m] @ inv(G[ot[m]])), Evi[m] @ (mirror4(To[m]) @ inv(G[ot[m]]))]
                src.append(ids[ot[m]])
            Gm, uvm = G[ot[ms]], uv[ms]
            costs = [float(view_costs(table, ovc[ms], Ev[ms] @ Tc[None], Gm, uvm, hv[ms]).sum()) for Tc in cands]
            Wn[c] = cands[int(np.argmin(costs))]
            won(trace, "frame", frames[c], costs, src)
        W = Wn
        Gn = G.copy()
        for j in range(NT):
            ms = [m for m in by_tag[j] if act[m]]
            if not tplaced[j] or not ms:
                continue
            cands = [G[j]]
            sm = [m for m in ms if seedable[m]]
            for kk in LR.top_k([area[m] for m in sm], MAX_CAND):
                m = sm[kk]
                Wi = inv(Ev[m] @ W[oc[m]])
                cands += [Wi @ To[m], Wi @ mirror4(To[m])]
            Wm, uvm = Wview(W, ms), uv[ms]
            costs = [float(view_costs(table, ovc[ms], Wm, np.broadcast_to(Tg, (len(ms), 4, 4)), uvm, hv[ms]).sum()) for Tg in cands]
            Gn[j] = cands[int(np.argmin(costs))]
            won(trace, "tag", ids[j], costs, [ids[j]] * (len(cands) // 2))
        G = Gn
    Gw = G[wt].copy()
    Mi = inv(Gw)
    W = W @ Gw[None]
    G = Mi[None] @ G
    G[wt] = np.eye(4)

    # flip test
    for j in range(NT):
        ms = [m for m in by_tag[j] if act[m]]
        if j == wt or not ms:
            continue
        Ws, uvs = list(Wview(W, ms)), [uv[m] for m in ms]
        T0, c0 = tag_lm(table, ovc[ms], G[j], Ws, uvs, ht[j])
        big = min(range(len(ms)), key=lambda kk: (-area[ms[kk]], kk))
        Wb = Ws[big]
        T1, c1 = tag_lm(table, ovc[ms], inv(Wb) @ mirror4(Wb @ G[j]), Ws, uvs, ht[j])
        G[j] = T1 if c1 < c0 else T0
        if trace is not None and c1 < c0:
            trace.setdefault("flipped", []).append(ids[j])

    # behind the camera, dropped frames, mapped tags
    for m in range(M):
        if act[m]:
            Wv = Ev[m] @ W[oc[m]]
            Pm = (obj3(hv[m]) @ G[ot[m]][:3, :3].T + G[ot[m]][:3, 3]) @ Wv[:3, :3].T + Wv[:3, 3]
            act[m] = bool((Pm[:, 2] > BEHIND_MARGIN).all())
            if trace is not None and not act[m]:
                trace.setdefault("behind", []).append(ids[ot[m]])
    cstat = np.where(cplaced, 0, 5)
    for c in range(NC):
        if cplaced[c] and len({int(ot[m]) for m in by_cam[c] if act[m]}) < 2:
            cstat[c] = 3
            act[by_cam[c]] = False
    mapped = np.array([j == wt or act[by_tag[j]].any() for j in range(NT)], dtype=bool)
    n_obs = int(act.sum())

    # the joint LM
    status = 0
    cost0 = cost = 0.0
    it = 0
    n_soft = 0
    cams_used = [c for c in range(NC) if cstat[c] == 0]
    free_tags = [j for j in range(NT) if mapped[j] and j != wt]
    if n_obs == 0:
        status = 1
    else:
        cam_col = np.full(NC, -1)
        tag_col = np.full(NT, -1)
        for i, c in enumerate(cams_used):
            cam_col[c] = 6 * i
        for i, j in enumerate(free_tags):
            tag_col[j] = 6 * (len(cams_used) + i)
        npar = 6 * (len(cams_used) + len(free_tags))
        a = np.flatnonzero(act)
        if reverse:
            a = a[::-1]

        def lin(Wx, Gx):
            return joint_linearise(table, Wx, Gx, oc[a], ot[a], ovc[a], uv[a], hv[a], cam_col, tag_col, npar, k, trace)

        allv = np.arange(M)
        seed_obs = view_costs(table, ovc, Wview(W, allv), G[ot], uv, hv, k)
        cost, H, g = lin(W, G)
        cost0 = cost
        lam = 1e-3
        while it < max_iters:
            it += 1
            A = H.copy()
            A[np.diag_indices(npar)] += lam * np.maximum(np.diag(H), 1e-12)
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                status = 2
                break
            d = solve_triangular(L, solve_triangular(L, -g, lower=True), lower=True, trans='T')
            Wn, Gn = W.copy(), G.copy()
            for c in cams_used:
                Wn[c] = gn_oracle.apply_update(W[c], d[cam_col[c]:cam_col[c] + 6])
            for j in free_tags:
                Gn[j] = gn_oracle.apply_update(G[j], d[tag_col[j]:tag_col[j] + 6])
            cn, Hn, gn = lin(Wn, Gn)
            if cn < cost:
                stop = cost - cn < 1e-12 * cost
                if trace is not None:
                    trace.setdefault("decreases", []).append((cost - cn) / cost)
                W, G, cost, H, g = Wn, Gn, cn, Hn, gn
                lam = max(lam * 0.1, 1e-12)
                if stop:
                    break
            else:
                lam *= 10
        if status == 0 and not np.isfinite(cost):
            status = 3
        if k > 0:
            rho, w, over, s, ok = corner_terms(table, ovc, Wview(W, allv), G[ot], uv, hv, k)
        if status == 0 and k > 0:
            wmin = w.min(axis=1)
            n_soft = int((over.any(axis=1) & act).sum())
            slot_weight[ovc[act], ofr[act], osl[act]] = wmin[act]
            if trace is not None:
                trace["margin"] = min(trace.get("margin", np.inf), margin(s[act], ok[act], k))
        elif status == 0:
            slot_weight[ovc[act], ofr[act], osl[act]] = 1.0
        if status == 0 and with_std:
            if k > 0:
                inl = ~over[act]
                n_in = int(inl.sum())
                dof = 2 * n_in - 6 * len(cams_used) - 6 * len(free_tags)
                s2 = float(np.where(ok[act], s[act] * s[act], LR.BEHIND_COST)[inl].sum()) / dof if dof > 0 else 0.0
            else:
                dof = 8 * n_obs - 6 * len(cams_used) - 6 * len(free_tags)
                s2 = cost / dof if dof > 0 else 0.0
            Li = solve_triangular(np.linalg.cholesky(H), np.eye(npar), lower=True)    # diag(H^-1)_i = |L^-1 e_i|^2
            Hid = (Li * Li).sum(axis=0)
            for j in free_tags:
                tag_std[ids[j]] = np.sqrt(s2 * Hid[tag_col[j]:tag_col[j] + 6])
        fin = view_costs(table, ovc, Wview(W, allv), G[ot], uv, hv, k)

    # records
    for c, f in enumerate(frames):
        na = int(act[by_cam[c]].sum())
        st = int(cstat[c])
        if st == 0 and status != 0:
            st = 4
        poses["status"][f] = st
        poses["seed_slot"][f] = seed_slot[c]
        poses["n_tags"][f] = na if st in (0, 4) else 0
        poses["n_rejected"][f] = npart[f] - (na if st in (0, 4) else 0)
        if st in (0, 4):
            poses["T"][f] = inv(W[c])
            if na and n_obs:
                poses["rms_px"][f] = np.sqrt(sum(fin[m] for m in by_cam[c] if act[m]) / (4.0 * na))
                poses["rms_seed_px"][f] = np.sqrt(sum(seed_obs[m] for m in by_cam[c] if act[m]) / (4.0 * na))
    for j in range(NT):
        if mapped[j] and status == 0:
            out_map["T"][ids[j]] = G[j][:3].ravel()
            out_map["valid"][ids[j]] = 1
            out_map["size"][ids[j]] = sizes[ids[j]]
    res["cost_seed"], res["cost"] = cost0, cost
    if n_obs:
        res["rms_px"], res["rms_seed_px"] = np.sqrt(cost / (4.0 * n_obs)), np.sqrt(cost0 / (4.0 * n_obs))
    res["n_frames_used"] = len(cams_used) if status == 0 else 0
    res["n_tags"] = int(mapped.sum()) if status == 0 else 0
    res["n_obs"] = n_obs
    res["n_obs_dropped"] = M - n_obs
    res["iterations"] = it
    res["status"] = status
    res["n_soft"] = n_soft
    return res, out_map, tag_std, poses, slot_weight
