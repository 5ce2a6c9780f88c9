"""Each kernel of the pose-graph back-end's linear algebra (csrc/k_gn.inc, k_map_std) as its own NumPy statement on the inputs
that kernel reads (TEST INFRASTRUCTURE).  Where a check needs more than double the work is done in np.longdouble; np.linalg
has no long-double routines, so the Cholesky, the triangular solves and the 6 x 6 inverse are plain loops, vectorised by row.

Every sum comes with the sum of its absolute terms and the number of products in it: the componentwise backward bounds of
the GPU tests (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3, 8 and 10) are gamma_k times that sum."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
NB = 48    # GN_NB: columns per block of the device's Cholesky


def gamma(k):
    return k * U / (1 - k * U)


def ld(a):
    return np.asarray(a, dtype=LD)


def worst(err, bound):
    """the largest |err| / bound over the entries; an error where the bound is 0 counts as infinite"""
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    ok = bound > 0
    r = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    return np.inf if (err[~ok] > 0).any() else r


# ---- dense: A = L L^T, L y = b, L^T x = y, diag(A^-1) ----------------------------------------------------------------

def cholesky(A, dtype=LD):
    """Lower factor of the symmetric A (lower triangle read), column by column; (L, j) with j the first pivot that is not
    positive, or None."""
    A = np.asarray(A, dtype=dtype)
    n = len(A)
    L = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return L, j
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L, None


def solve_lower(L, b):
    """L y = b by rows; b (n,) or (n, k)"""
    L = np.asarray(L)
    y = np.zeros(np.shape(b), dtype=np.result_type(L.dtype, np.asarray(b).dtype))
    for i in range(len(L)):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def solve_upper_t(L, y):
    """L^T x = y by rows, last first"""
    L = np.asarray(L)
    x = np.zeros(np.shape(y), dtype=np.result_type(L.dtype, np.asarray(y).dtype))
    for i in range(len(L) - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def diag_inverse(L):
    """diag((L L^T)^-1)_i = |L^-1 e_i|^2"""
    Li = solve_lower(L, np.eye(len(L), dtype=L.dtype))
    return (Li * Li).sum(axis=0)


def back_substitution(L, Linv, y, dtype=LD, with_bound=False):
    """k_gn_trisolve's operation on the factor, the diagonal blocks' inverses and y it reads: from the last block to the first,
    x_b = Linv_b^T r_b with r_b = y_b less L_{b'b}^T x_b' of every later block b'.  with_bound: also the running componentwise
    forward bound of that recursion in arithmetic with unit roundoff u, E_b = |Linv_b^T| (gamma_{n+52} (|y_b| + sum |L_{b'b}^T||x_b'|)
    + sum |L_{b'b}^T| E_b'): the products of one entry (at most n from the rows below, 48 of the block, 4 to spare) and the error
    the later blocks hand down.  It is relative to every entry's own terms, so it holds row by row whatever the rows' scales."""
    L, y = np.asarray(L, dtype=dtype), np.asarray(y, dtype=dtype)
    n = len(L)
    r, ra, E = y.copy(), np.abs(y), np.zeros(n, dtype=dtype)
    x = np.zeros(n, dtype=dtype)
    g = dtype(gamma(n + 52))
    for bi in range(len(blocks(n)) - 1, -1, -1):
        k0, nb = blocks(n)[bi]
        Lit = np.asarray(Linv[bi], dtype=dtype)[:nb, :nb].T
        x[k0:k0 + nb] = Lit @ r[k0:k0 + nb]
        E[k0:k0 + nb] = np.abs(Lit) @ (g * ra[k0:k0 + nb] + E[k0:k0 + nb])
        P = L[k0:k0 + nb, :k0].T
        r[:k0] -= P @ x[k0:k0 + nb]
        ra[:k0] += np.abs(P) @ np.abs(x[k0:k0 + nb])
        E[:k0] += np.abs(P) @ E[k0:k0 + nb]    # until block b is solved E[b] collects what the later blocks hand down
    return (x, E) if with_bound else x


def blocks(n):
    """(k0, nb) of every block column"""
    return [(k0, min(NB, n - k0)) for k0 in range(0, n, NB)]


def cond2(M):
    s = np.linalg.svd(np.asarray(M, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1])


def block_cond(L):
    """kappa_b = max over the diagonal blocks of cond_2(L_bb)"""
    return max(cond2(L[k0:k0 + nb, k0:k0 + nb]) for k0, nb in blocks(len(L)))


def dense_ratios(A, b, L, y, x, Linv, var):
    """Error over bound of every dense quantity, for a factor L, y = L^-1 b, x, the Linv blocks and var = diag(A^-1) as some
    arithmetic with unit roundoff 2^-53 returned them; residuals in long double.  The bounds:
      factor  |A - L L^T| <= gamma_{n+4} |L||L^T| on the lower triangle
      y       |b - L y| <= gamma_{n+4} |L||y|
      Linv    |L_bb Linv_b - I| <= gamma_52 |L_bb||Linv_b|, and a partial block's padding exactly the identity
      x       |L^T x - y|_inf <= gamma_{n+52} (1 + kappa_b) |L|_inf |x|_inf
      x_fwd   |x - back_substitution(L, Linv, y)| <= its running componentwise bound: the norm-wise bar above is relative to
              the largest rows of a system whose rows differ in scale by 10^6 and does not see an error in a small row
      var     |var_i - ref_i| <= gamma_{2n+52} (1 + kappa_b) cond_2(L) ref_i,  ref_i = |L^-1 e_i|^2 in long double"""
    n = len(A)
    Al, Ll, yl, xl = ld(np.tril(A)), ld(np.tril(L)), ld(y), ld(x)
    aL = np.abs(Ll)

    out = {}
    out["factor"] = worst(np.tril(Al - Ll @ Ll.T), gamma(n + 4) * np.tril(aL @ aL.T))
    out["y"] = worst(ld(b) - Ll @ yl, gamma(n + 4) * (aL @ np.abs(yl)))
    r = 0.0
    pad_ok = True
    for bi, (k0, nb) in enumerate(blocks(n)):
        Lbb, Lib = Ll[k0:k0 + nb, k0:k0 + nb], ld(Linv[bi])
        r = max(r, worst(Lbb @ Lib[:nb, :nb] - np.eye(nb), gamma(52) * (np.abs(Lbb) @ np.abs(Lib[:nb, :nb]))))
        pad = np.array(Linv[bi], dtype=np.float64)
        pad[:nb, :nb] = np.eye(nb)
        pad_ok = pad_ok and np.array_equal(pad, np.eye(NB)) and not np.triu(Linv[bi], 1).any()
    out["Linv"] = r
    out["Linv_pad"] = 0.0 if pad_ok else np.inf
    kb = block_cond(L)
    out["x"] = float(np.abs(Ll.T @ xl - yl).max() / (gamma(n + 52) * (1 + kb) * aL.sum(axis=1).max() * np.abs(xl).max() + LD(1e-300)))
    xr, E = back_substitution(Ll, Linv, yl, with_bound=True)
    out["x_fwd"] = worst(xl - xr, E)
    ref = diag_inverse(Ll)
    out["var"] = worst(ld(var) - ref, gamma(2 * n + 52) * (1 + kb) * cond2(L) * ref)
    return out


# ---- the observation blocks --------------------------------------------------------------------------------------------

def obs_blocks(Jc, Jt, r, corners=None, dtype=LD):
    """D (M, 12, 13) = [J^T J | J^T r] and the costs (M,) from gn_oracle.linearize's Jc, Jt (M, 8, 6) and r (M, 8); with the
    corners (M, 8) also the absolute sums of the bound: (|J|^T |J| with |r_k| replaced by |u_k| + |corner_k|, and the
    cost's sum of (|u_k| + |corner_k|)^2): the residual is a difference of two pixel coordinates."""
    J = np.concatenate([np.asarray(Jc, dtype=dtype), np.asarray(Jt, dtype=dtype)], axis=2)      # (M, 8, 12)
    r = np.asarray(r, dtype=dtype)
    Jr = np.concatenate([J, r[:, :, None]], axis=2)
    D = np.einsum('mki,mkj->mij', J, Jr)
    cost = (r * r).sum(axis=1)
    if corners is None:
        return D, cost
    c = np.abs(np.asarray(corners, dtype=dtype).reshape(len(r), 8))
    ra = np.abs(r + np.asarray(corners, dtype=dtype).reshape(len(r), 8)) + c
    Da = np.einsum('mki,mkj->mij', np.abs(J), np.concatenate([np.abs(J), ra[:, :, None]], axis=2))
    return D, cost, Da, (ra * ra).sum(axis=1)


def lists(P, L, obs_cam, obs_tag):
    """the observations of every camera and of every tag in observation order, and the (camera, tag) -> observation table"""
    oc, ot = np.asarray(obs_cam, dtype=np.int64), np.asarray(obs_tag, dtype=np.int64)
    of = -np.ones((P, L), dtype=np.int64)
    of[oc, ot] = np.arange(len(oc))
    return [np.flatnonzero(oc == f) for f in range(P)], [np.flatnonzero(ot == j) for j in range(L)], of


def damp(s, lam):
    """k_gn_reduce_cam's and k_gn_schur's damping of a diagonal entry s"""
    return s + lam * (s if s > 1e-12 else type(s)(1e-12))


def inv6(H):
    """the inverse of the symmetric positive definite 6 x 6 H by Cholesky (gn_inv6: Hinv = L^-T L^-1); (Hinv, L_H), or
    (None, None) if a pivot is not positive"""
    Lh, bad = cholesky(H, dtype=np.asarray(H).dtype)
    if bad is not None:
        return None, None
    Li = solve_lower(Lh, np.eye(6, dtype=Lh.dtype))
    return Li.T @ Li, Lh


def reduce_cams(D, cams, lam, dtype=LD):
    """Per camera, from the blocks D and the damping: the damped H_cc, its inverse (zero for a camera without observations or
    a block that is not positive definite), g_c, and per observation T_fj = H_cc^-1 W_fj.  Returns dict(H, H_abs (the absolute terms of H's sums), Hinv, LH, gc, gc_abs,
    Tfj, Tfj_abs)."""
    D = np.asarray(D, dtype=dtype)
    P, M = len(cams), len(D)
    H, Hinv, LH, Ha = np.zeros((P, 6, 6), dtype), np.zeros((P, 6, 6), dtype), np.zeros((P, 6, 6), dtype), np.zeros((P, 6, 6), dtype)
    gc, gca = np.zeros((P, 6), dtype), np.zeros((P, 6), dtype)
    Tfj, Tfa = np.zeros((M, 6, 6), dtype), np.zeros((M, 6, 6), dtype)
    for f, idx in enumerate(cams):
        for m in idx:    # observation order
            H[f] += D[m, :6, :6]
            Ha[f] += np.abs(D[m, :6, :6])
            gc[f] += D[m, :6, 12]
            gca[f] += np.abs(D[m, :6, 12])
        for i in range(6):
            Ha[f, i, i] += np.abs(damp(H[f, i, i], dtype(lam)) - H[f, i, i])
            H[f, i, i] = damp(H[f, i, i], dtype(lam))
        if len(idx) == 0:
            continue
        Hi, Lh = inv6(H[f])
        if Hi is None:
            continue
        Hinv[f], LH[f] = Hi, Lh
        for m in idx:
            Tfj[m] = Hi @ D[m, :6, 6:12]
            Tfa[m] = np.abs(Hi) @ np.abs(D[m, :6, 6:12])
    return dict(H=H, H_abs=Ha, Hinv=Hinv, LH=LH, gc=gc, gc_abs=gca, Tfj=Tfj, Tfj_abs=Tfa)


def tfj(D, Hinv, obs_cam, dtype=LD):
    """T_fj = Hinv_f W_fj from given inverses, with the absolute sums"""
    D, Hinv = np.asarray(D, dtype=dtype), np.asarray(Hinv, dtype=dtype)
    Hm = Hinv[np.asarray(obs_cam, dtype=np.int64)]
    return np.einsum('mik,mkj->mij', Hm, D[:, :6, 6:12]), np.einsum('mik,mkj->mij', np.abs(Hm), np.abs(D[:, :6, 6:12]))


def schur(D, Tfj, Hinv, gc, obs_cam, tags, obs_of, fixed_tag, lam, dtype=LD):
    """The reduced system over the tags: S = H_ll (damped) - sum_f W_fj^T T_fj2 and rhs = -g_l + sum_f W_fj^T Hinv_f g_f, with the
    6 x 6 identity and rhs 0 on the rows and columns of the fixed tag and of every tag without observations.  Returns
    (S, rhs, S_abs, rhs_abs, S_k, rhs_k): values, sums of absolute terms, products per entry."""
    D, Tfj, Hinv, gc = (np.asarray(a, dtype=dtype) for a in (D, Tfj, Hinv, gc))
    oc = np.asarray(obs_cam, dtype=np.int64)
    L = len(tags)
    n = 6 * L
    S, Sa, Sk = np.zeros((n, n), dtype), np.zeros((n, n), dtype), np.zeros((n, n), np.int64)
    rhs, ra, rk = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, np.int64)
    frozen = [j == fixed_tag or len(tags[j]) == 0 for j in range(L)]
    for j in range(L):
        rj = slice(6 * j, 6 * j + 6)
        if frozen[j]:
            S[rj, rj] = np.eye(6)
            continue
        for j2 in range(L):
            if frozen[j2]:
                continue
            cj = slice(6 * j2, 6 * j2 + 6)
            s, sa, k = np.zeros((6, 6), dtype), np.zeros((6, 6), dtype), 0
            if j == j2:
                for m in tags[j]:
                    s += D[m, 6:12, 6:12]
                    sa += np.abs(D[m, 6:12, 6:12])
                k += len(tags[j]) + 1
                for a in range(6):
                    d = damp(s[a, a], dtype(lam))
                    sa[a, a] += np.abs(d - s[a, a])
                    s[a, a] = d
            for m in tags[j]:
                m2 = obs_of[oc[m], j2]
                if m2 < 0:
                    continue
                s -= D[m, :6, 6:12].T @ Tfj[m2]
                sa += np.abs(D[m, :6, 6:12]).T @ np.abs(Tfj[m2])
                k += 6
            S[rj, cj], Sa[rj, cj], Sk[rj, cj] = s, sa, k
        for m in tags[j]:
            f = oc[m]
            rhs[rj] -= D[m, 6:12, 12]
            ra[rj] += np.abs(D[m, 6:12, 12])
        for m in tags[j]:
            f = oc[m]
            rhs[rj] += D[m, :6, 6:12].T @ (Hinv[f] @ gc[f])
            ra[rj] += np.abs(D[m, :6, 6:12]).T @ (np.abs(Hinv[f]) @ np.abs(gc[f]))
        rk[rj] = len(tags[j]) * (1 + 6 * (1 + 6))
    return S, rhs, Sa, ra, Sk, rk


def camera_steps(D, Hinv, gc, dG, cams, obs_tag, dtype=LD):
    """d_f = Hinv_f (-g_f - sum_j W_fj dG_j); (steps (P, 6), absolute sums, products per entry (P,))"""
    D, Hinv, gc, dG = (np.asarray(a, dtype=dtype) for a in (D, Hinv, gc, dG))
    ot = np.asarray(obs_tag, dtype=np.int64)
    P = len(cams)
    d, da, k = np.zeros((P, 6), dtype), np.zeros((P, 6), dtype), np.zeros(P, np.int64)
    for f, idx in enumerate(cams):
        r, ra = -gc[f], np.abs(gc[f])
        for m in idx:
            r = r - D[m, :6, 6:12] @ dG[ot[m]]
            ra = ra + np.abs(D[m, :6, 6:12]) @ np.abs(dG[ot[m]])
        d[f], da[f], k[f] = Hinv[f] @ r, np.abs(Hinv[f]) @ ra, 6 * len(idx) + 1 + 6
    return d, da, k


def exp_rot(w, with_k2=False):
    """I + sin(theta) K + (1 - cos(theta)) K^2 for w = theta k; with_k2: also K^2 (zero for w = 0)"""
    w = np.asarray(w)
    th = np.sqrt((w * w).sum())
    if th < 1e-300:
        R, K2 = np.eye(3, dtype=w.dtype), np.zeros((3, 3), dtype=w.dtype)
    else:
        k = w / th
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=w.dtype)
        K2 = K @ K
        R = np.eye(3, dtype=w.dtype) + np.sin(th) * K + (1 - np.cos(th)) * K2
    return (R, K2) if with_k2 else R


def apply_update12(P12, d, dtype=LD):
    """gn_oracle.apply_update on a pose packed as the kernels hold it (R row-major, then t): (exp(d) * pose, the entry sums
    |exp(omega)| |pose| + |v| the bound is relative to, and the same sums with |K^2| in place of |exp(omega)|: cos(theta) is a
    number next to 1 known to 2 u absolute, so 1 - cos(theta) carries 2 u however small it is, and with it every entry of
    exp(omega) carries 2 u |K^2|, which the relative bound does not hold where the entry sum is small)"""
    P12, d = np.asarray(P12, dtype=dtype), np.asarray(d, dtype=dtype)
    R, K2 = exp_rot(d[:3], with_k2=True)
    Rs, ts = P12[:9].reshape(3, 3), P12[9:]
    out = np.concatenate([(R @ Rs).reshape(9), R @ ts + d[3:]])
    mag = np.concatenate([(np.abs(R) @ np.abs(Rs)).reshape(9), np.abs(R) @ np.abs(ts) + np.abs(d[3:])])
    mag2 = np.concatenate([(np.abs(K2) @ np.abs(Rs)).reshape(9), np.abs(K2) @ np.abs(ts)])
    return out, mag, mag2


def pack12(T):
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[..., :3, :3].reshape(T.shape[:-2] + (9,)), T[..., :3, 3]], axis=-1)


def rigid_inverse12(T):
    """camera<-world packed, from world<-camera 4 x 4, as gn_rigid_inverse forms it (R^T, -R^T t by rows, left to right)"""
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros(T.shape[:-2] + (12,))
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :9] = Rt.reshape(T.shape[:-2] + (9,))
    for r in range(3):
        out[..., 9 + r] = -((Rt[..., r, 0] * T[..., 0, 3] + Rt[..., r, 1] * T[..., 1, 3]) + Rt[..., r, 2] * T[..., 2, 3])
    return out


def step_ratios(c, D, Hinv, gc, Tfj, S, rhs):
    """error over bound of the per-camera and Schur quantities, each against its statement in long double on the given inputs
    (gc: gamma_{n_f} on the sums in observation order; Hinv: |Hinv H - I| <= gamma_24 |Hinv||L_H||L_H^T| + gamma_{n_f+2} |Hinv| H_abs
    with H and its factor rebuilt in long double from D and H_abs the absolute terms of H's sums and damping -- the kernel
    inverts the H it summed in double in observation order, which is the long-double H only to gamma_{n_f+2} H_abs, and under
    strong damping (L_H nearly diagonal) |L_H||L_H^T| does not cover that where an off-diagonal sum cancels; exactly 0 for a
    camera without observations; Tfj, S, rhs: gamma_{k+8} times the sum of
    absolute terms, k the products in the entry; the rows and columns of frozen tags exactly the identity, rhs 0 there)"""
    cams, tags, of = lists(c["P"], c["L"], c["obs_cam"], c["obs_tag"])
    ref = reduce_cams(D, cams, c["lam"])
    out = {}

    nf = np.array([max(len(i), 1) for i in cams])
    out["gc"] = worst(ld(gc) - ref["gc"], gamma(nf)[:, None] * ref["gc_abs"])
    r = 0.0
    for f, idx in enumerate(cams):
        if len(idx) == 0:
            r = max(r, 0.0 if not np.asarray(Hinv[f]).any() else np.inf)
            continue
        Lh = np.abs(ref["LH"][f])
        aH = np.abs(ld(Hinv[f]))
        r = max(r, worst(ld(Hinv[f]) @ ref["H"][f] - np.eye(6), gamma(24) * (aH @ Lh @ Lh.T) + gamma(len(idx) + 2) * (aH @ ref["H_abs"][f])))
    out["Hinv"] = r
    T, Ta = tfj(D, Hinv, c["obs_cam"])
    out["Tfj"] = worst(ld(Tfj) - T, gamma(6 + 8) * Ta)
    Sr, rr, Sa, ra, Sk, rk = schur(D, Tfj, Hinv, gc, c["obs_cam"], tags, of, c["fixed_tag"], c["lam"])
    frozen = np.repeat([j == c["fixed_tag"] or len(tags[j]) == 0 for j in range(c["L"])], 6)
    exact = np.array_equal(np.asarray(S)[frozen], np.eye(len(frozen))[frozen]) and np.array_equal(np.asarray(S)[:, frozen], np.eye(len(frozen))[:, frozen]) \
        and not np.asarray(rhs)[frozen].any()
    out["frozen_rows"] = 0.0 if exact else np.inf
    out["S"] = worst(ld(S) - Sr, gamma(Sk + 8) * Sa)
    out["rhs"] = worst(ld(rhs) - rr, gamma(rk + 8) * ra)
    return out


def update_ratios(c, W12, G12, D, Hinv, gc, dG, Wn, Gn):
    """error over bound of the trial poses some arithmetic returned for the poses (W12, G12), blocks, inverses, gradients and
    tag steps dG it read.  Gn: exp(dG_j) G_j to 64 u of the entry sums |exp(omega)||G| + |v| plus 2 u of the |K^2| sums
    (apply_update12: the absolute error of 1 - cos(theta)).  Wn: exp(d_f) W_f with d_f the
    camera step in long double from the same inputs, to the same plus what the step's own bound
    e = gamma_{k+8} |Hinv|(|g| + sum |W_fj||dG_j|) moves the pose to first order: |e_omega|_1 max|column| on the rotation
    part, |e_omega|_1 max|t| + |e_v| on t."""
    cams, tags, of = lists(c["P"], c["L"], c["obs_cam"], c["obs_tag"])
    d, da, k = camera_steps(D, Hinv, gc, dG, cams, c["obs_tag"])
    out = {"Wn": 0.0, "Gn": 0.0}
    for f in range(c["P"]):
        ref, mag, mag2 = apply_update12(W12[f], d[f])
        e = gamma(int(k[f]) + 8) * da[f]
        colmax = np.abs(W12[f][:9]).reshape(3, 3).max(axis=0)
        move = np.concatenate([np.tile(e[:3].sum() * colmax, 3), e[:3].sum() * np.abs(W12[f][9:]).max() + e[3:]])
        out["Wn"] = max(out["Wn"], worst(ld(Wn[f]) - ref, 64 * U * mag + 2 * U * mag2 + move))
    for j in range(c["L"]):
        ref, mag, mag2 = apply_update12(G12[j], np.asarray(dG).reshape(-1, 6)[j])
        out["Gn"] = max(out["Gn"], worst(ld(Gn[j]) - ref, 64 * U * mag + 2 * U * mag2))
    return out
