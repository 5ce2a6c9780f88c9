"""Named, seeded cases for the kernel-by-kernel tests of the pose-graph back-end's linear algebra (TEST INFRASTRUCTURE):
dense matrices for asl_debug_gn_cholesky at the block edges of the blocked Cholesky, the back substitution and k_map_std,
and small pose-graph problems for asl_debug_gn_step.  tests/test_gn_ref.py checks that every case has what its name claims."""
import numpy as np

from gn_problem import make_problem

NB = 48
# tags L (n = 6 L): one block with nb = 6 .. 48; a second block of 6, 42 and 48 columns and a third of 6; n = 258, first
# past k_map_std's 256-thread stride; 510 and 516; 534, the first size at which k_gn_trisolve's strided loop runs
# (k0 = 528 > 512 threads), with a last block of 6; 576 = twelve whole blocks, and 582
DENSE_L = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 43, 85, 86, 89, 96, 97)
# the same with the last tag not frozen, where that tag is the whole last block: otherwise the partial last block is the
# identity and its unknowns are 0, and neither the factorisation's last step nor what the back substitution carries from the
# last block to the rows above (at n = 534: the strided loop's only work) would show
FREE_LAST_L = (9, 17, 89, 97)
DENSE_CASES = tuple((L, False) for L in DENSE_L) + tuple((L, True) for L in FREE_LAST_L)
NOT_PD = ("block0", "middle", "partial_last")


def frozen_tags(L):
    """the "frozen" tags of a dense case (6 x 6 identity rows and columns, as k_gn_schur leaves them for the fixed tag and
    unobserved tags): in the first block, in the last block, and on each side of the first seam (tags 7 and 8, rows 42..47 and
    48..53).  Small cases keep at least one ordinary tag."""
    if L == 1:
        return ()
    if L == 2:
        return (0,)
    return tuple(sorted({0, L - 1} | ({7, 8} if L >= 9 else set())))


def dense_case_id(case):
    return "L%d%s" % (case[0], "_free_last" if case[1] else "")


def dense_case(L, free_last=False, seed=None, frozen=None):
    """A = D (B B^T + n I) D with B random, D diagonal with entries over 1e-3 .. 1e3 in a 3 + 3 pattern per tag (a real S mixes
    rotation and translation scales like that), frozen tags as identity rows and columns; b random, zero on frozen rows."""
    n = 6 * L
    rng = np.random.default_rng(7000 + L if seed is None else seed)
    B = rng.standard_normal((n, n))
    M = B @ B.T + n * np.eye(n)
    e = rng.permutation(np.linspace(3.0, 1.0, L))    # per tag: rotation rows 10^e, translation rows 10^-e, e in [1, 3]
    d = np.concatenate([np.concatenate([np.full(3, 10.0 ** ej), np.full(3, 10.0 ** -ej)]) for ej in e])
    A = d[:, None] * M * d[None, :]
    A = 0.5 * (A + A.T)
    b = rng.standard_normal(n) * d
    if frozen is None:
        frozen = tuple(j for j in frozen_tags(L) if not (free_last and j == L - 1))
    frozen = tuple(frozen)
    for j in frozen:
        r = slice(6 * j, 6 * j + 6)
        A[r, :] = 0.0
        A[:, r] = 0.0
        A[r, r] = np.eye(6)
        b[r] = 0.0
    return dict(name="dense_" + dense_case_id((L, free_last)), L=L, n=n, A=A, b=b, frozen=frozen, n_blocks=(n + NB - 1) // NB, last_nb=n - (n - 1) // NB * NB)


def not_pd_case(where):
    """dense_case(17) (n = 102: blocks of 48, 48 and 6 columns) with one pivot made negative: the diagonal entry is lowered
    so that the pivot the factorisation meets there is minus half of what it was.  Everything else stays ordinary (the last
    tag is not frozen here: it is the whole partial block)."""
    c = dense_case(17, frozen=(0, 7, 8))
    j = {"block0": 20, "middle": 60, "partial_last": 99}[where]
    Lf = np.linalg.cholesky(c["A"])
    A = c["A"].copy()
    A[j, j] -= 1.5 * Lf[j, j] ** 2
    c.update(name="notpd_" + where, A=A, pivot=j, pivot_block=j // NB)
    return c


# ---- problems for asl_debug_gn_step ------------------------------------------------------------------------------------

PROBLEM_L = (1, 2, 3, 8, 9, 17)
LAMBDAS = (1e-3, 1e-9, 1e3)
VARIANTS = ("unobserved_tag", "empty_camera", "single_obs_camera", "single_obs_tag")
_BASE = {}


def base_problem(L):
    """make_problem(P = 6, L, seed 40 + L, noise 0.25), computed once"""
    if L not in _BASE:
        _BASE[L] = make_problem(P=6, L=L, seed=40 + L, noise=0.25)
    return _BASE[L]


def fixed_tags(L):
    return tuple(sorted({0, L // 2, L - 1}))


def _drop(pr, keep):
    out = dict(pr)
    for k in ("obs_cam", "obs_tag", "obs_corners"):
        out[k] = pr[k][keep]
    return out


def variant_target(L, fixed_tag, variant):
    """the tag or camera a variant changes: an unobserved tag next to the first seam where there is one (tag 7 of 9: rows
    42..47), otherwise the last tag, never the fixed one; camera 1; the single-observation tag likewise not the fixed one"""
    if variant in ("empty_camera", "single_obs_camera"):
        return 1
    t = 7 if L == 9 else L - 1
    if variant == "single_obs_tag":
        t = 8 if L == 9 else max(L - 2, 0)
    while t == fixed_tag:
        t = (t + 1) % L
    return t


def problem_case(L, fixed_tag, lam, variant=None):
    pr = base_problem(L)
    oc, ot = pr["obs_cam"], pr["obs_tag"]
    target = None
    if variant is not None:
        target = variant_target(L, fixed_tag, variant)
        m = np.arange(len(oc))
        if variant == "unobserved_tag":
            keep = ot != target
        elif variant == "empty_camera":
            keep = oc != target
        elif variant == "single_obs_camera":
            keep = (oc != target) | (m == np.flatnonzero(oc == target)[0])
        elif variant == "single_obs_tag":
            keep = (ot != target) | (m == np.flatnonzero(ot == target)[0])
        else:
            raise ValueError(variant)
        pr = _drop(pr, keep)
    name = "L%d_fix%d_lam%g" % (L, fixed_tag, lam) + ("_" + variant if variant else "")
    return dict(pr, name=name, L=L, P=len(pr["cam0"]), fixed_tag=fixed_tag, lam=lam, variant=variant, target=target, tag_size=10.0)


def problem_case_ids():
    """(L, fixed_tag, lambda, variant): every L x fixed_tag x lambda, and every variant once per L at fixed_tag L // 2 and
    lambda 1e-3 (with one tag, L = 1, only the cameras can be changed)"""
    ids = [(L, f, lam, None) for L in PROBLEM_L for f in fixed_tags(L) for lam in LAMBDAS]
    for L in PROBLEM_L:
        for v in VARIANTS:
            if L == 1 and v in ("unobserved_tag", "single_obs_tag"):
                continue
            ids.append((L, L // 2, 1e-3, v))
    return ids


def case_name(c):
    return "L%d_fix%d_lam%g" % c[:3] + ("_" + c[3] if c[3] else "")
