"""The pose-graph back-end's linear algebra kernel by kernel (csrc/k_gn.inc, k_map_std), through asl_debug_gn_cholesky and
asl_debug_gn_step: each kernel against its own statement (tests/gn_ref.py) on the inputs that kernel read, as read back from
the device, so that every link is sharp and no bar has to absorb the conditioning of the whole system.  Every bound is a
componentwise backward bound of textbook form (Higham, Accuracy and Stability of Numerical Algorithms, ch. 8 and 10) with
u = 2^-53 and gamma_k = k u / (1 - k u); every residual is evaluated in long double (a float64 L @ L.T has rounding of the
size of the bound).  tests/test_gn_ref.py holds NumPy's float64 results to the same bounds.  The end-to-end additions at the
bottom go through asl_gn_solve itself against gn_oracle.solve with the project's bars (cost 1e-9 relative, poses 1e-6).

Largest error over bound seen on the device per quantity: DESIGN.md section 7."""
import numpy as np
import pytest

import gn_cases as C
import gn_ref as R
from gn_problem import G

pytestmark = pytest.mark.gpu

PROBLEMS = C.problem_case_ids()
SEEN = {}    # quantity -> largest error / bound over the module's cases (printed when the module is done: pytest -s)


@pytest.fixture(scope="module")
def det(gpu_detector):
    yield gpu_detector
    print("\nlargest error / bound:", {k: "%.3g" % v for k, v in sorted(SEEN.items())})


def note(ratios):
    for k, v in ratios.items():
        SEEN[k] = max(SEEN.get(k, 0.0), float(v))


def rows_of(tags):
    return np.concatenate([np.arange(6 * j, 6 * j + 6) for j in tags] + [np.zeros(0, dtype=np.int64)])


# ---- asl_debug_gn_cholesky: k_gn_chol_diag / _panel / _update, k_gn_trisolve, k_map_std ------------------------------------

@pytest.mark.parametrize("case", C.DENSE_CASES, ids=C.dense_case_id)
def test_dense_factor_solve_and_variance(det, case):
    """gn_ref.dense_ratios' bounds on the device's factor, y = L^-1 b (the right-hand side riding as row n), the Linv blocks, x
    and var; a frozen tag's rows of the factor are the identity's and y and x are exactly 0 there."""
    c = C.dense_case(*case)
    out = det.debug_gn_cholesky(c["A"], c["b"])
    assert out["fail"] == 0
    for k in ("L", "y", "x", "Linv", "var"):
        assert np.isfinite(out[k]).all(), k
    assert not np.triu(out["L"], 1).any()
    fr = rows_of(c["frozen"])
    assert np.array_equal(out["L"][fr], np.eye(c["n"])[fr]) and not out["y"][fr].any() and not out["x"][fr].any()
    assert np.array_equal(out["var"][fr], np.ones(len(fr)))
    ratios = R.dense_ratios(c["A"], c["b"], out["L"], out["y"], out["x"], out["Linv"], out["var"])
    print(c["name"], {k: "%.3g" % v for k, v in ratios.items()})
    note(ratios)
    assert max(ratios.values()) < 1, ratios


@pytest.mark.parametrize("where", C.NOT_PD)
def test_not_positive_definite_is_flagged(det, where):
    """one negative pivot in block 0, in a middle block, in the partial last block: the call returns and the flag is set"""
    c = C.not_pd_case(where)
    out = det.debug_gn_cholesky(c["A"], c["b"])
    assert out["fail"] == 1
    ok = C.dense_case(17, frozen=c["frozen"])
    assert det.debug_gn_cholesky(ok["A"], ok["b"])["fail"] == 0


# ---- asl_debug_gn_step: k_gn_linearize, k_gn_cost, k_gn_reduce_cam, k_gn_schur, the factor, k_gn_trisolve, k_gn_update -----

def device_inputs(c):
    """the poses as asl_gn_solve hands them to the kernels: W camera<-world by gn_rigid_inverse, G packed"""
    W12, G12 = R.rigid_inverse12(c["cam0"]), R.pack12(c["tag0"])
    W44 = np.tile(np.eye(4), (len(W12), 1, 1))
    W44[:, :3, :3], W44[:, :3, 3] = W12[:, :9].reshape(-1, 3, 3), W12[:, 9:]
    return W12, G12, W44


@pytest.mark.parametrize("case", PROBLEMS, ids=C.case_name)
def test_step_kernel_by_kernel(det, case):
    """One damped step, every kernel against its statement on what it read:
      D, cost     |D_ij - ref| <= 64 u (|J|^T |J|)_ij with gn_oracle.linearize's J and r at the device's poses; in the column J^T r
                  |r_k| is replaced by |u_k| + |corner_k| (the residual is a difference of two pixel coordinates of about 10^3);
                  the observation costs and their sum in the same form, the sum also to 1e-9 relative
      gc, Hinv, Tfj, S, rhs   gn_ref.step_ratios, from the device's own D, Hinv, gc and Tfj
      dG          the factor and substitution bounds of the dense test on the device's S and rhs: asl_debug_gn_cholesky on them
                  runs the same launches, so its x is dG bit for bit and brings the factor and y along
      Wn, Gn      gn_ref.update_ratios: exp(d) pose to 64 u of the entry sums, with d_f the camera step from the device's D, Hinv, gc
                  and dG in long double and its own bound carried into the pose
    Two terms the first derivation missed are named where they enter (gn_ref.step_ratios: the double sums behind H_cc under
    Hinv's bound; gn_ref.apply_update12: the absolute error of 1 - cos(theta)); NumPy's float64 arithmetic exceeds the bounds
    without them on the same cases (lambda = 1e3), see DESIGN.md section 7.
      the fixed tag, an unobserved tag and a camera without observations keep their poses bit for bit."""
    c = C.problem_case(*case)
    P, L, lam = c["P"], c["L"], c["lam"]
    o = det.debug_gn_step(c["cam0"], c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"], c["fixed_tag"], lam)
    assert o["fail"] == 0
    W12, G12, W44 = device_inputs(c)
    cams, tags, of = R.lists(P, L, c["obs_cam"], c["obs_tag"])
    ratios = {}

    cost, r, Jc, Jt = G.linearize(W44, c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"])
    Dr, cr, Da, ca = R.obs_blocks(Jc, Jt, r, corners=c["obs_corners"])
    ratios["D"] = R.worst(R.ld(o["D"]) - Dr, 64 * R.U * Da)
    ratios["cost_obs"] = R.worst(R.ld(o["cost_obs"]) - cr, 64 * R.U * ca)
    ratios["cost"] = R.worst(R.ld(o["cost"][0]) - cr.sum(), 64 * R.U * ca.sum())
    assert abs(o["cost"][0] - cost) <= 1e-9 * cost

    ratios.update(R.step_ratios(c, o["D"], o["Hinv"], o["gc"], o["Tfj"], o["S"], o["rhs"]))

    dense = det.debug_gn_cholesky(o["S"], o["rhs"])
    assert dense["fail"] == 0 and np.array_equal(dense["x"], o["dG"].reshape(-1))
    dr = R.dense_ratios(o["S"], o["rhs"], dense["L"], dense["y"], dense["x"], dense["Linv"], dense["var"])
    ratios.update({"step_" + k: v for k, v in dr.items()})

    ratios.update(R.update_ratios(c, W12, G12, o["D"], o["Hinv"], o["gc"], o["dG"], o["Wn"], o["Gn"]))

    still_tags = [j for j in range(L) if j == c["fixed_tag"] or len(tags[j]) == 0]
    still_cams = [f for f in range(P) if len(cams[f]) == 0]
    assert c["fixed_tag"] in still_tags
    if c["variant"] == "unobserved_tag":
        assert c["target"] in still_tags
    if c["variant"] == "empty_camera":
        assert still_cams == [c["target"]]
    for j in still_tags:
        assert o["Gn"][j].tobytes() == G12[j].tobytes() and not o["dG"][j].any(), j
    for f in still_cams:
        assert o["Wn"][f].tobytes() == W12[f].tobytes() and not o["Hinv"][f].any(), f
    moved = [j for j in range(L) if j not in still_tags]
    assert all(o["dG"][j].any() for j in moved) and all(o["Wn"][f].tobytes() != W12[f].tobytes() for f in range(P) if f not in still_cams)

    print(c["name"], {k: "%.3g" % v for k, v in ratios.items()})
    note(ratios)
    assert max(ratios.values()) < 1, ratios


def test_wanted_items_only(det):
    """an item that is not wanted is not written, and the wanted ones do not depend on which others were asked for"""
    c = C.problem_case(3, 1, 1e-3)
    args = (c["cam0"], c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"], c["fixed_tag"], c["lam"])
    full = det.debug_gn_step(*args)
    part = det.debug_gn_step(*args, want=("S", "dG"))
    assert sorted(part) == ["S", "dG", "fail"] and np.array_equal(part["S"], full["S"]) and np.array_equal(part["dG"], full["dG"])


# ---- end to end: asl_gn_solve against gn_oracle.solve ----------------------------------------------------------------------

def solve_both(det, c, iters):
    args = (c["cam0"], c["tag0"], c["obs_cam"], c["obs_tag"], c["obs_corners"], c["K"], c["tag_size"], c["fixed_tag"])
    return G.solve(*args, iters=iters), det.gn_solve(*args, iters=iters)


def close(ref, got):
    (cam_o, tag_o, st_o), (cam_g, tag_g, st_g) = ref, got
    assert abs(st_g[0] - st_o[0]) <= 1e-9 * st_o[0] and abs(st_g[1] - st_o[1]) <= 1e-9 * st_o[1], (st_g, st_o)
    assert st_g[2] == st_o[2]
    assert np.abs(tag_g - tag_o).max() < 1e-6 and np.abs(cam_g - cam_o).max() < 1e-6


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("L,fixed_tag", sorted({(L, f) for L in C.PROBLEM_L for f in (L // 2, L - 1)}))
def test_solve_first_steps_with_other_fixed_tags(det, L, fixed_tag, iters):
    """one and two iterations, where no later step can make up for a wrong one, with the gauge tag in the middle and last"""
    c = C.problem_case(L, fixed_tag, 1e-3)
    ref, got = solve_both(det, c, iters)
    close(ref, got)
    assert got[1][fixed_tag].tobytes() == np.asarray(c["tag0"][fixed_tag], dtype=np.float64).tobytes()


@pytest.mark.parametrize("variant", ["unobserved_tag", "empty_camera"])
@pytest.mark.parametrize("L", [L for L in C.PROBLEM_L if L > 1])
def test_solve_leaves_the_unobserved_alone(det, L, variant):
    """an unobserved tag's pose comes back bit-identical, a camera's without observations within 1e-12 (it passes through two
    rigid inversions)"""
    c = C.problem_case(L, L // 2, 1e-3, variant)
    ref, got = solve_both(det, c, 2)
    close(ref, got)
    assert got[2][2] >= 1
    if variant == "unobserved_tag":
        assert got[1][c["target"]].tobytes() == np.asarray(c["tag0"][c["target"]], dtype=np.float64).tobytes()
    else:
        assert np.abs(got[0][c["target"]] - c["cam0"][c["target"]]).max() <= 1e-12


@pytest.mark.parametrize("L", [1, 9])
def test_solve_zero_iterations(det, L):
    c = C.problem_case(L, L // 2, 1e-3)
    ref, (cam, tag, st) = solve_both(det, c, 0)
    close(ref, (cam, tag, st))
    assert st[0] == st[1] and st[2] == 0
    assert tag.tobytes() == np.asarray(c["tag0"], dtype=np.float64).tobytes() and np.abs(cam - c["cam0"]).max() <= 1e-12
