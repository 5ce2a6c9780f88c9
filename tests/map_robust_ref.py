"""NumPy statement of the tag-map reconstruction with a robust (Huber) corner loss (asl_map_robust_frames_device /
asl_map_robust_batch, aprilslam_amd/csrc/k_map.inc).  Test infrastructure; tests/map_ref.py states the plain call and
everything that is not named here.

  seeding  gather, chain, the two reseed sweeps, gauge, flip test and behind-camera test are map_ref's, with squared costs.
  LM       huber_px = k > 0, in pixels, on every corner's raw residual r = (r0, r1), s = |r|: s <= k costs s^2 with weight 1,
           s > k costs 2 k s - k^2 with weight k / s; a corner at z <= 1e-9 costs 1e12, adds no row and is never over.  The
           corner adds weight J^T J and weight J^T r to the normal equations (iteratively reweighted Gauss-Newton, no
           second-order term of the loss).  The robust cost stands wherever map_ref's LM has the squared one: cost_seed,
           cost, every trial, the accept rule and the 1e-12 stop, and the per-frame and result rms_px / rms_seed_px, which
           are sqrt(sum of corner costs / corners).  Damping, schedule, statuses and the sets in the solve are map_ref's.
  soft     at the returned poses an observation's weight is the smallest of its four corner weights, in (0, 1]; it is
           soft with a weight < 1.  n_soft counts them; slot_weight (n_frames, max_tags) holds the weights, 0 for every
           slot that is not in the solve, and for every slot (with n_soft 0) when the status is not 0.
  std      the diagonal of the inverse of the weighted undamped normal matrix at the solution, times
           sigma^2 = sum of s^2 over the corners not over k / (2 n_in - 6 frames - 6 (tags - 1)), n_in their number (a
           corner at z <= 1e-9 is one of them, with its 1e12); 0 if the denominator is <= 0.  The factor leaves the
           outliers' linear tails out, so one bad slot does not inflate every tag's std; the truncation at k biases it
           slightly low.
  k = 0    the plain computation: map_ref.map_frames' output byte for byte, n_soft 0, weight 1 for the slots in the solve.

reverse (a rounding perturbation for the tests): the LM's sums run over the observations in reversed order.
trace (a dict, optional) receives "margin", the smallest |s - k| over every corner of every linearisation and of the
final weights, and "flipped" as map_ref's.
"""
import numpy as np
from scipy.linalg import solve_triangular

import localize_ref as LR
import map_ref as MR
from aprilslam_amd._lib import CAM_POSE_DTYPE, MAP_RESULT_DTYPE, MAP_TAG_DTYPE
from map_ref import BEHIND_MARGIN, MAX_CAND, MAX_MAP_TAGS, SWEEPS, gn_oracle, inv, mirror4, obj3, obs_costs, rec4, tag_lm


def corner_terms(cam, W, G, uv, h, k):
    """per corner of n observations (W (n, 4, 4) camera<-world, G (n, 4, 4) world<-tag, uv (n, 4, 2)): (cost, weight, over,
    s, in front), each (n, 4); k = 0: the squared loss"""
    Xw = np.einsum('nij,kj->nki', G[:, :3, :3], obj3(h)) + G[:, None, :3, 3]
    P = (np.einsum('nij,nkj->nki', W[:, :3, :3], Xw) + W[:, None, :3, 3]).reshape(-1, 3)
    ok = P[:, 2] > LR.Z_MIN
    e, s = np.zeros(len(P)), np.zeros(len(P))
    if ok.any():
        r = LR.project(cam, P[ok]) - uv.reshape(-1, 2)[ok]
        e[ok] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        s[ok] = np.sqrt(e[ok])
    over = ok & (s > k) if k > 0 else np.zeros(len(P), dtype=bool)
    w = np.ones(len(P))
    w[over] = k / s[over]
    rho = np.where(over, 2.0 * k * s - k * k, e)
    rho[~ok] = LR.BEHIND_COST
    sh = (len(W), 4)
    return rho.reshape(sh), w.reshape(sh), over.reshape(sh), s.reshape(sh), ok.reshape(sh)


def margin(s, ok, k):
    """smallest |s - k| over the corners in front"""
    return float(np.abs(s[ok] - k).min()) if ok.any() else np.inf


def robust_linearise(cam, W, G, oc, ot, uv, h, cam_col, tag_col, n_par, k, trace=None):
    """map_ref.joint_linearise with the loss: (cost, H, g), H and g of the weighted rows; k = 0 is joint_linearise itself"""
    if k == 0.0:
        return MR.joint_linearise(cam, W, G, oc, ot, uv, h, cam_col, tag_col, n_par)
    X = obj3(h)
    M = len(oc)
    q = np.einsum('mij,kj->mki', G[ot][:, :3, :3], X) + G[ot][:, None, :3, 3]
    P = np.einsum('mij,mkj->mki', W[oc][:, :3, :3], q) + W[oc][:, None, :3, 3]
    pr, Jp, ok = MR._project_many(cam, P.reshape(-1, 3))
    r = (pr - uv.reshape(-1, 2)) * ok[:, None]
    e = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    s = np.sqrt(e)
    over = ok & (s > k)
    w = np.ones(len(s))
    w[over] = k / s[over]
    rho = np.where(over, 2.0 * k * s - k * k, e)
    cost = float(rho.sum()) + LR.BEHIND_COST * float((~ok).sum())
    if trace is not None:
        trace["margin"] = min(trace.get("margin", np.inf), margin(s, ok, k))
    sw = np.sqrt(w)
    Jp = Jp * (ok * sw)[:, None, None]
    r = r * sw[:, None]
    Pf, qf = P.reshape(-1, 3), q.reshape(-1, 3)
    Jc = np.concatenate([np.cross(Pf[:, None, :], Jp), Jp], axis=2)
    a = np.einsum('nri,nij->nrj', Jp, np.repeat(W[oc][:, :3, :3], 4, axis=0))
    Jt = np.concatenate([np.cross(qf[:, None, :], a), a], axis=2)
    Jc, Jt, r8 = Jc.reshape(M, 8, 6), Jt.reshape(M, 8, 6), r.reshape(M, 8)
    ccol, tcol = cam_col[oc], tag_col[ot]
    H, g = np.zeros((n_par, n_par)), np.zeros(n_par)
    i6 = np.arange(6)

    def add(rc, cc, blk, sel):
        if sel.any():
            np.add.at(H, (rc[sel][:, None, None] + i6[None, :, None], cc[sel][:, None, None] + i6[None, None, :]), blk[sel])

    cm, tm = ccol >= 0, tcol >= 0
    add(ccol, ccol, np.einsum('mri,mrj->mij', Jc, Jc), cm)
    add(tcol, tcol, np.einsum('mri,mrj->mij', Jt, Jt), tm)
    ct = np.einsum('mri,mrj->mij', Jc, Jt)
    add(ccol, tcol, ct, cm & tm)
    add(tcol, ccol, ct.transpose(0, 2, 1), cm & tm)
    if cm.any():
        np.add.at(g, ccol[cm][:, None] + i6, np.einsum('mri,mr->mi', Jc, r8)[cm])
    if tm.any():
        np.add.at(g, tcol[tm][:, None] + i6, np.einsum('mri,mr->mi', Jt, r8)[tm])
    return cost, H, g


def robust_obs_costs(cam, W, G, uv, h, k):
    """map_ref.obs_costs under the loss: (n,)"""
    if k == 0.0:
        return obs_costs(cam, W, G, uv, h)
    return corner_terms(cam, W, G, uv, h, k)[0].sum(axis=1)


def map_frames(obs, n_ids, K, dist, tag_size, world_id=-1, huber_px=0.0, max_iters=30, with_std=True, trace=None, reverse=False):
    """map_ref.map_frames' four (the result's last int is n_soft) and slot_weight (n_frames, max_tags)"""
    k = float(huber_px)
    if not (k >= 0 and np.isfinite(k)):
        raise ValueError("huber_px must be >= 0 and finite")
    obs = np.asarray(obs)
    F, S = obs.shape
    cam = LR.camera(K, dist)
    h = LR.half_size(tag_size)
    res = np.zeros((), dtype=MAP_RESULT_DTYPE)
    out_map = np.zeros(n_ids, dtype=MAP_TAG_DTYPE)
    tag_std = np.zeros((n_ids, 6))
    poses = np.zeros(F, dtype=CAM_POSE_DTYPE)
    poses["T"] = np.eye(4)
    poses["seed_slot"] = -1
    poses["status"] = 1
    slot_weight = np.zeros((F, S))

    # gather
    part = np.zeros((F, S), dtype=bool)
    for f in range(F):
        seen = set()
        for s in range(S):
            i, fl = int(obs["id"][f, s]), int(obs["flags"][f, s])
            if (fl & 1) and 0 <= i < n_ids and i not in seen:
                part[f, s] = True
                seen.add(i)
    npart = part.sum(axis=1)
    frames = [f for f in range(F) if npart[f] >= 2]
    ids = sorted({int(obs["id"][f, s]) for f in frames for s in range(S) if part[f, s]})
    tag_of = {i: j for j, i in enumerate(ids)}
    ob = [(c, tag_of[int(obs["id"][f, s])], f, s) for c, f in enumerate(frames) for s in range(S) if part[f, s]]
    oc = np.array([o[0] for o in ob], dtype=np.int64)
    ot = np.array([o[1] for o in ob], dtype=np.int64)
    ofr = np.array([o[2] for o in ob], dtype=np.int64)
    osl = np.array([o[3] for o in ob], dtype=np.int64)
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
    uv = np.stack([obs["corners"][f, s].astype(np.float64).reshape(4, 2) for f, s in zip(ofr, osl)]) if M else np.zeros((0, 4, 2))
    To = [rec4(obs["T"][f, s]) for f, s in zip(ofr, osl)]
    seedable = np.array([bool(obs["flags"][f, s] & 2) for f, s in zip(ofr, osl)], dtype=bool)
    area = np.array([LR.corner_area(obs["corners"][f, s]) for f, s in zip(ofr, osl)])
    by_cam = [np.flatnonzero(oc == c) for c in range(NC)]
    by_tag = [np.flatnonzero(ot == j) for j in range(NT)]

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
                m = min(cand, key=lambda m: (-area[m], ot[m]))
                W[c] = To[m] @ inv(G[ot[m]])
                cplaced[c] = True
                seed_slot[c] = osl[m]
                changed = True
        for j in range(NT):
            if tplaced[j]:
                continue
            cand = [m for m in by_tag[j] if seedable[m] and cplaced[oc[m]]]
            if cand:
                m = min(cand, key=lambda m: (-area[m], oc[m]))
                G[j] = inv(W[oc[m]]) @ To[m]
                tplaced[j] = True
                changed = True
    act = cplaced[oc] & tplaced[ot] if M else np.zeros(0, dtype=bool)

    # sweeps
    for _ in range(SWEEPS):
        Wn = W.copy()
        for c in range(NC):
            ms = [m for m in by_cam[c] if act[m]]
            if not cplaced[c] or not ms:
                continue
            cands = [W[c]]
            sm = [m for m in ms if seedable[m]]
            for kk in LR.top_k([area[m] for m in sm], MAX_CAND):
                m = sm[kk]
                cands += [To[m] @ inv(G[ot[m]]), mirror4(To[m]) @ inv(G[ot[m]])]
            Gm, uvm = G[ot[ms]], uv[ms]
            costs = [float(obs_costs(cam, np.broadcast_to(Tc, (len(ms), 4, 4)), Gm, uvm, h).sum()) for Tc in cands]
            Wn[c] = cands[int(np.argmin(costs))]
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
                Wi = inv(W[oc[m]])
                cands += [Wi @ To[m], Wi @ mirror4(To[m])]
            Wm, uvm = W[oc[ms]], uv[ms]
            costs = [float(obs_costs(cam, Wm, np.broadcast_to(Tg, (len(ms), 4, 4)), uvm, h).sum()) for Tg in cands]
            Gn[j] = cands[int(np.argmin(costs))]
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
        Ws, uvs = [W[oc[m]] for m in ms], [uv[m] for m in ms]
        T0, c0 = tag_lm(cam, G[j], Ws, uvs, h)
        big = min(range(len(ms)), key=lambda kk: (-area[ms[kk]], kk))
        Wb = Ws[big]
        T1, c1 = tag_lm(cam, inv(Wb) @ mirror4(Wb @ G[j]), Ws, uvs, h)
        G[j] = T1 if c1 < c0 else T0
        if trace is not None and c1 < c0:
            trace.setdefault("flipped", []).append(ids[j])

    # behind the camera, dropped frames, mapped tags
    X = obj3(h)
    for m in range(M):
        if act[m]:
            Pm = (X @ G[ot[m]][:3, :3].T + G[ot[m]][:3, 3]) @ W[oc[m]][:3, :3].T + W[oc[m]][:3, 3]
            act[m] = bool((Pm[:, 2] > BEHIND_MARGIN).all())
    cstat = np.where(cplaced, 0, 5)
    for c in range(NC):
        if cplaced[c] and act[by_cam[c]].sum() < 2:
            cstat[c] = 3
            act[by_cam[c]] = False
    mapped = np.array([j == wt or act[by_tag[j]].any() for j in range(NT)], dtype=bool)
    n_obs = int(act.sum())

    # the joint LM under the loss
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
            return robust_linearise(cam, Wx, Gx, oc[a], ot[a], uv[a], h, cam_col, tag_col, npar, k, trace)

        seed_obs = robust_obs_costs(cam, W[oc], G[ot], uv, h, k)
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
                W, G, cost, H, g = Wn, Gn, cn, Hn, gn
                lam = max(lam * 0.1, 1e-12)
                if stop:
                    break
            else:
                lam *= 10
        if status == 0 and not np.isfinite(cost):
            status = 3
        if k > 0:
            rho, w, over, s, ok = corner_terms(cam, W[oc], G[ot], uv, h, k)
        if status == 0 and k > 0:
            wmin = w.min(axis=1)
            n_soft = int((over.any(axis=1) & act).sum())
            slot_weight[ofr[act], osl[act]] = wmin[act]
            if trace is not None:
                trace["margin"] = min(trace.get("margin", np.inf), margin(s[act], ok[act], k))
        elif status == 0:
            slot_weight[ofr[act], osl[act]] = 1.0
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
        fin = robust_obs_costs(cam, W[oc], G[ot], uv, h, k)

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
