"""tests/gn_ref.py and tests/gn_cases.py on the CPU: the statements chained together are gn_oracle.lm_step, every case has the
edges its name claims, and correct float64 arithmetic (NumPy, SciPy) meets every bound the GPU tests put on the device."""
import numpy as np
import pytest
import scipy.linalg as sl

import gn_cases as C
import gn_ref as R
from gn_problem import G

PROBLEMS = C.problem_case_ids()


def chain(c, dtype=R.LD):
    """one damped step of case c through the statements of gn_ref, each fed with the one before"""
    W = [np.linalg.inv(T) for T in c["cam0"]]
    cost, r, Jc, Jt = G.linearize(W, c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"])
    D, _ = R.obs_blocks(Jc, Jt, r, dtype=dtype)
    cams, tags, of = R.lists(c["P"], c["L"], c["obs_cam"], c["obs_tag"])
    rc = R.reduce_cams(D, cams, c["lam"], dtype=dtype)
    S, rhs, _, _, _, _ = R.schur(D, rc["Tfj"], rc["Hinv"], rc["gc"], c["obs_cam"], tags, of, c["fixed_tag"], c["lam"], dtype=dtype)
    Lf, bad = R.cholesky(S, dtype=dtype)
    assert bad is None
    dG = R.solve_upper_t(Lf, R.solve_lower(Lf, rhs)).reshape(c["L"], 6)
    dW, _, _ = R.camera_steps(D, rc["Hinv"], rc["gc"], dG, cams, c["obs_tag"], dtype=dtype)
    return dict(S=S, rhs=rhs, dG=dG, dW=dW, cams=cams, tags=tags, H=rc["H"])


@pytest.mark.parametrize("case", PROBLEMS, ids=C.case_name)
def test_statements_compose_to_lm_step(case):
    """The chain in long double against gn_oracle.lm_step (float64, np.linalg.solve on the kept rows).  What separates them is
    lm_step's own rounding: a backward-stable float64 solve or inverse is off by about cond_2 u relative to the result's norm,
    and lm_step both solves the kept system and inverts every damped camera block, so the bar is 64 u kappa |step|_inf with
    kappa the larger of cond_2(S_kept) and the camera blocks' cond_2.  Frozen rows are exact."""
    c = C.problem_case(*case)
    ch = chain(c)
    W = [np.linalg.inv(T) for T in c["cam0"]]
    args = (W, c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"], c["fixed_tag"], c["lam"])
    _, dW, dG = G.lm_step(*args)
    S, b, keep = G.reduced_system(*args)
    assert not ch["dG"].reshape(-1)[~keep].any() and not dG.reshape(-1)[~keep].any()
    if keep.any():
        kappa = R.cond2(S[np.ix_(keep, keep)])
        # the kept part of the statement's S is the oracle's S there
        Sk = np.asarray(ch["S"], dtype=np.float64)[np.ix_(keep, keep)]
        assert np.abs(Sk - S[np.ix_(keep, keep)]).max() <= 1e-9 * np.abs(S[np.ix_(keep, keep)]).max()
    else:
        kappa = 1.0
        assert np.array_equal(np.asarray(ch["S"], dtype=np.float64), np.eye(6 * c["L"])) and not ch["rhs"].any()
    kappa = max([kappa] + [R.cond2(ch["H"][f]) for f, idx in enumerate(ch["cams"]) if len(idx)])
    step = max(np.abs(dG).max(), np.abs(dW).max())
    bar = 64 * R.U * kappa * step
    err = max(float(np.abs(ch["dG"] - dG).max()), float(np.abs(ch["dW"] - dW).max()))
    print("%s: cond %.3g, error / bar %.3g" % (c["name"], kappa, err / bar))
    assert err <= bar


@pytest.mark.parametrize("L", C.PROBLEM_L)
def test_problem_cases_have_their_structure(L):
    pr = C.base_problem(L)
    P = len(pr["cam0"])
    assert P == 6 and len(pr["tag0"]) == L
    per_tag, per_cam = np.bincount(pr["obs_tag"], minlength=L), np.bincount(pr["obs_cam"], minlength=P)
    assert per_tag.min() >= 2 and per_cam.min() >= 1, (per_tag, per_cam)
    assert len(set(zip(pr["obs_cam"].tolist(), pr["obs_tag"].tolist()))) == len(pr["obs_cam"])
    assert C.fixed_tags(L) == tuple(sorted({0, L // 2, L - 1}))
    for case in PROBLEMS:
        if case[0] != L or case[3] is None:
            continue
        c = C.problem_case(*case)
        t, v = c["target"], c["variant"]
        pt, pc = np.bincount(c["obs_tag"], minlength=L), np.bincount(c["obs_cam"], minlength=P)
        if v == "unobserved_tag":
            assert t != c["fixed_tag"] and pt[t] == 0 and len(c["obs_tag"]) == len(pr["obs_tag"]) - per_tag[t]
        elif v == "empty_camera":
            assert pc[t] == 0 and len(c["obs_cam"]) == len(pr["obs_cam"]) - per_cam[t]
        elif v == "single_obs_camera":
            assert pc[t] == 1 and len(c["obs_cam"]) == len(pr["obs_cam"]) - per_cam[t] + 1
        else:
            assert t != c["fixed_tag"] and pt[t] == 1 and len(c["obs_tag"]) == len(pr["obs_tag"]) - per_tag[t] + 1
        if v in ("unobserved_tag", "single_obs_tag"):
            assert (np.delete(pt, t) == np.delete(per_tag, t)).all()
    if L == 9:    # the unobserved tag sits left of the first seam, a fixed tag right of it
        assert C.variant_target(9, 4, "unobserved_tag") == 7 and 8 in C.fixed_tags(9)
    if L == 1:    # the only tag is fixed: S = I, rhs = 0, the cameras move alone
        ch = chain(C.problem_case(1, 0, 1e-3))
        assert np.array_equal(np.asarray(ch["S"], dtype=np.float64), np.eye(6)) and not ch["rhs"].any() and not ch["dG"].any()
        assert np.abs(ch["dW"]).max() > 0


def test_problem_conditioning_spans_what_the_issue_states():
    """cond_2 of the kept system over the base cases: from about 2e4 up to about 5e10 (the latter at lambda = 1e-9)"""
    conds = {}
    for case in PROBLEMS:
        if case[3] is not None or case[0] == 1:
            continue
        c = C.problem_case(*case)
        W = [np.linalg.inv(T) for T in c["cam0"]]
        S, b, keep = G.reduced_system(W, c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"], c["fixed_tag"], c["lam"])
        conds[case] = R.cond2(S[np.ix_(keep, keep)])
    lo, hi = min(conds, key=conds.get), max(conds, key=conds.get)
    print("cond_2: %.3g at %s .. %.3g at %s" % (conds[lo], C.case_name(lo), conds[hi], C.case_name(hi)))
    assert conds[lo] < 1e5 and 1e10 < conds[hi] < 1e12 and hi[2] == 1e-9


def test_dense_sizes_reach_every_edge():
    assert C.DENSE_L == (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 43, 85, 86, 89, 96, 97) and max(C.DENSE_L) == 97
    assert C.FREE_LAST_L == (9, 17, 89, 97) and all(6 * L % 48 == 6 for L in C.FREE_LAST_L) and len(C.DENSE_CASES) == 22
    shape = {L: (C.dense_case(L)["n_blocks"], C.dense_case(L)["last_nb"]) for L in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 89, 96, 97)}
    assert [shape[L] for L in range(1, 9)] == [(1, 6 * L) for L in range(1, 9)]              # one block, nb = 6 .. 48
    assert shape[9] == (2, 6) and shape[15] == (2, 42) and shape[16] == (2, 48) and shape[17] == (3, 6)
    assert shape[89] == (12, 6) and shape[96] == (12, 48) and shape[97] == (13, 6)
    assert 6 * 43 == 258 > 256 >= 6 * 42                                                      # first size past k_map_std's stride
    # k_gn_trisolve's strided loop (i = tid + 512 < k0) runs first at k0 = 528: the last block of n = 534; not at 85, 86
    last_k0 = {L: R.blocks(6 * L)[-1][0] for L in C.DENSE_L}
    assert [L for L in C.DENSE_L if last_k0[L] > 512] == [89, 96, 97] and last_k0[89] == 528 and last_k0[86] == 480
    # rem == 1 (only the right-hand-side row below the block: no trailing update) is every case's last block; a single
    # block has nothing else
    for L in C.DENSE_L:
        k0, nb = R.blocks(6 * L)[-1]
        assert 6 * L + 1 - k0 - nb == 1


@pytest.mark.parametrize("case", C.DENSE_CASES, ids=C.dense_case_id)
def test_dense_case_and_bounds_in_float64(case):
    """The case is what it says (symmetric, frozen rows the identity with b = 0 there and on both sides of the first seam, D's
    spread), and NumPy's float64 factor and SciPy's substitutions meet every bound of the GPU tests with ratio < 1."""
    L, free_last = case
    c = C.dense_case(L, free_last)
    A, b, n = c["A"], c["b"], c["n"]
    assert A.shape == (n, n) and np.array_equal(A, A.T) and n == 6 * L
    assert c["n_blocks"] == len(R.blocks(n)) and c["last_nb"] == R.blocks(n)[-1][1]
    fz = c["frozen"]
    if L >= 3:
        assert 0 in fz and (L - 1 in fz) != free_last
    if free_last:    # the last tag is the whole last block, and nothing of it is the identity's
        assert c["last_nb"] == 6 and np.abs(A[-6:, -6:]).min() > 0 and np.count_nonzero(A[-6:, :-6]) >= 6 * 6 * (L - 1 - len(fz)) and np.abs(b[-6:]).min() > 0
    if L >= 9:
        assert 7 in fz and (8 in fz or (free_last and L == 9)) and (6 * 7 + 5) // 48 == 0 and (6 * 8) // 48 == 1
    assert len(fz) < L
    for j in fz:
        rows = np.arange(6 * j, 6 * j + 6)
        assert np.array_equal(A[rows], np.eye(n)[rows]) and not b[rows].any()
    free = np.setdiff1d(np.arange(n), np.concatenate([np.arange(6 * j, 6 * j + 6) for j in fz] + [np.zeros(0, int)]))
    d = np.sqrt(np.diag(A)[free])
    assert d.max() / d.min() > 50 and 1e-4 < d.min() and d.max() < 1e5 and np.abs(b[free]).min() > 0    # 3 + 3 rows at 10^+-e, e >= 1
    ratios = float64_ratios(A, b)
    print(c["name"], {k: "%.3g" % v for k, v in ratios.items()})
    assert max(ratios.values()) < 1, ratios


def float64_ratios(A, b):
    n = len(A)
    Lf = np.linalg.cholesky(A)
    y = sl.solve_triangular(Lf, b, lower=True)
    Linv = np.zeros((len(R.blocks(n)), R.NB, R.NB))
    for bi, (k0, nb) in enumerate(R.blocks(n)):
        Linv[bi] = np.eye(R.NB)
        Linv[bi, :nb, :nb] = sl.solve_triangular(Lf[k0:k0 + nb, k0:k0 + nb], np.eye(nb), lower=True)
    x = R.back_substitution(Lf, Linv, y, dtype=np.float64)    # the blocked substitution through the explicit inverses
    assert np.abs(x - sl.solve_triangular(Lf.T, y, lower=False)).max() <= 1e-6 * np.abs(x).max()
    Li = sl.solve_triangular(Lf, np.eye(n), lower=True)
    return R.dense_ratios(A, b, Lf, y, x, Linv, (Li * Li).sum(axis=0))


@pytest.mark.parametrize("where", C.NOT_PD)
def test_not_positive_definite_cases_fail_where_they_say(where):
    c = C.not_pd_case(where)
    A, j = c["A"], c["pivot"]
    assert np.array_equal(A, A.T) and c["n"] == 102 and [nb for _, nb in R.blocks(102)] == [48, 48, 6]
    assert c["pivot_block"] == {"block0": 0, "middle": 1, "partial_last": 2}[where] == j // 48
    assert j // 6 not in c["frozen"]
    Lf, bad = R.cholesky(A)
    assert bad == j                                  # every pivot before it is positive, this one is not
    ok = C.dense_case(17, frozen=c["frozen"])
    piv = float(R.cholesky(ok["A"])[0][j, j]) ** 2
    got = float(ld_pivot(A, Lf, j))
    assert abs(got + 0.5 * piv) < 1e-6 * piv         # minus half of what it was: ordinary in size, nothing overflows
    assert np.isfinite(A).all() and np.abs(A - ok["A"]).astype(bool).sum() == 1


def ld_pivot(A, Lf, j):
    return R.ld(A[j, j]) - Lf[j, :j] @ Lf[j, :j]


@pytest.mark.parametrize("case", PROBLEMS, ids=C.case_name)
def test_problem_bounds_in_float64(case):
    """One step with every statement evaluated in float64 on the float64 output of the one before (what the device does, up to
    the order inside a sum) meets the GPU tests' bounds: gc, Hinv, Tfj, S, rhs, the dense quantities of the real reduced
    system, the trial poses.  Without the two terms named in gn_ref.step_ratios and gn_ref.apply_update12 it does not, at
    lambda = 1e3: Hinv reaches 11 times its bound (L = 9) and Wn twice (L = 17, fixed tag 16)."""
    c = C.problem_case(*case)
    W12, G12 = R.rigid_inverse12(c["cam0"]), R.pack12(c["tag0"])
    W44 = np.tile(np.eye(4), (c["P"], 1, 1))
    W44[:, :3, :3], W44[:, :3, 3] = W12[:, :9].reshape(-1, 3, 3), W12[:, 9:]
    _, r, Jc, Jt = G.linearize(W44, c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"])
    D, _ = R.obs_blocks(Jc, Jt, r, dtype=np.float64)
    cams, tags, of = R.lists(c["P"], c["L"], c["obs_cam"], c["obs_tag"])
    r64 = R.reduce_cams(D, cams, c["lam"], dtype=np.float64)
    S, rhs = R.schur(D, r64["Tfj"], r64["Hinv"], r64["gc"], c["obs_cam"], tags, of, c["fixed_tag"], c["lam"], dtype=np.float64)[:2]
    ratios = R.step_ratios(c, D, r64["Hinv"], r64["gc"], r64["Tfj"], S, rhs)
    ratios.update(float64_ratios(S, rhs))
    Lf = np.linalg.cholesky(S)
    dG = sl.solve_triangular(Lf.T, sl.solve_triangular(Lf, rhs, lower=True), lower=False).reshape(-1, 6)
    d, _, _ = R.camera_steps(D, r64["Hinv"], r64["gc"], dG, cams, c["obs_tag"], dtype=np.float64)
    Wn = np.array([R.apply_update12(W12[f], d[f], dtype=np.float64)[0] for f in range(c["P"])])
    Gn = np.array([R.apply_update12(G12[j], dG[j], dtype=np.float64)[0] for j in range(c["L"])])
    ratios.update(R.update_ratios(c, W12, G12, D, r64["Hinv"], r64["gc"], dG, Wn, Gn))
    print(c["name"], {k: "%.3g" % v for k, v in ratios.items()})
    assert max(ratios.values()) < 1, ratios
