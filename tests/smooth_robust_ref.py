"""NumPy statement of the sequence localisation with a robust corner loss (asl_smooth_robust_sequences_device / _batch,
k_smooth_cand<true> and k_smooth_lin<true> of aprilslam_amd/csrc/k_smooth.inc over loc_corner<NE, true> of k_localize.inc).
It is smooth_ref.py's computation with one term changed: every taking-part corner's pixel residual r = (r0, r1) goes
through a Huber loss of threshold k = huber_px pixels (on the raw residual, before sigma_px).  With e = r0^2 + r1^2, s = sqrt(e):

    s <= k   rho = e                 wgt = 1          (the plain term)
    s >  k   rho = 2 k s - k^2       wgt = k / s
    z <= 1e-9   rho = 1e12, nothing added to H and g (as in localize_ref)

A frame's data cost is sum rho (divided by sigma_px^2 where |r_f|^2 is in smooth_ref), its H = sum wgt J^T J and g = sum
wgt J^T r over its corners, J the localisation's 2x6 rows: iteratively reweighted Gauss-Newton, no second-order term.  The
robust cost stands wherever the squared one does: the candidates' data costs in the seed chain, the cost after the chain,
every trial and the accept rule, cost_seed and cost; rms_px and rms_seed_px (per frame and in the result) are
sqrt(sum rho / corners), the plain RMS when no corner is over the threshold.  The motion prior, tridiag_solve, the LM
schedule, the stop rule and the fill of unposed frames are smooth_ref's, imported from there.

A slot is "soft" at a state if at least one of its four corners has wgt < 1 there (a corner behind the camera has none).
A frame's n_rejected is the number of its soft slots at the returned poses, the result's n_soft their sum; the count belongs
to the linearisation a trial commits, as the frame's pixel cost does.

Corner sums run in slot order, as the device's lanes hold them (reverse: in reversed slot order, a rounding perturbation).
huber_px = 0 is smooth_ref.smooth, byte for byte.  The covariance (smooth_cov) is smooth_cov_ref's factor / marginals over
the robust problem's blocks at the returned poses: a down-weighted corner contributes wgt of its information.
Test infrastructure, as smooth_ref.py is.
"""
import numpy as np

import localize_ref as LR
import pose_cov_ref as PC
import smooth_cov_ref as SCR
import smooth_ref as SR
from aprilslam_amd._lib import CAM_POSE_DTYPE, SMOOTH_RESULT_DTYPE


def corner_terms(cam, R, t, Xw, uv, k, jac=False):
    """per corner of one frame at (R, t): (rho, wgt, over, ok[, J (m, 2, 6) and r (m, 2) of the ok corners])"""
    P = Xw @ R.T + t
    ok = P[:, 2] > LR.Z_MIN
    rho, wgt, over = np.full(len(P), LR.BEHIND_COST), np.zeros(len(P)), np.zeros(len(P), dtype=bool)
    J = r = None
    if ok.any():
        p = P[ok]
        if jac:
            q, Jp = LR.project(cam, p, jac=True)
            J = np.concatenate([Jp @ LR.neg_skew(p), Jp], axis=2)
        else:
            q = LR.project(cam, p)
        r = q - uv[ok]
        e = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        s = np.sqrt(e)
        o = s > k
        safe = np.where(o, s, 1.0)
        wgt[ok] = np.where(o, k / safe, 1.0)
        rho[ok] = np.where(o, 2.0 * k * s - k * k, e)
        over[ok] = o
    return (rho, wgt, over, ok, J, r) if jac else (rho, wgt, over, ok)


class Problem(SR.Problem):
    """smooth_ref.Problem with the Huber loss of threshold huber_px on every corner (0: the plain problem)"""

    def __init__(self, obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, huber_px, reverse=False):
        super().__init__(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, reverse)
        self.k = float(huber_px)

    def data_cost(self, f, P):
        """the frame's robust pixel cost at P (not yet weighted by sigma_px)"""
        if self.k == 0.0 or self.pts[f] is None:
            return super().data_cost(f, P)
        return float(corner_terms(self.cam, P[0], P[1], *self.pts[f], self.k)[0].sum())

    def frame(self, f, P):
        """(cost, H, g, soft slots, wgt per corner, |r| per corner (nan behind the camera)) of frame f at P = (R, t)"""
        rho, wgt, over, ok, J, r = corner_terms(self.cam, P[0], P[1], *self.pts[f], self.k, jac=True)
        H, g = np.zeros((6, 6)), np.zeros(6)
        s = np.full(len(rho), np.nan)
        if ok.any():
            w = wgt[ok]
            H = (w[:, None, None] * (J[:, 0, :, None] * J[:, 0, None, :] + J[:, 1, :, None] * J[:, 1, None, :])).sum(axis=0)
            g = (w[:, None] * (J[:, 0, :] * r[:, 0:1] + J[:, 1, :] * r[:, 1:2])).sum(axis=0)
            s[ok] = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        return float(rho.sum()), H, g, int(over.reshape(-1, 4).any(axis=1).sum()), wgt, s

    def linearise(self, P):
        """smooth_ref's, the corner terms weighted; "soft": the frames' soft-slot counts at P"""
        lin = super().linearise(P)
        lin["soft"] = np.zeros(self.n, dtype=np.int64)
        if self.k == 0.0:
            return lin
        for f in range(self.n):
            if self.pts[f] is not None:
                lin["c"][f], lin["H"][f], lin["g"][f], lin["soft"][f] = self.frame(f, P[f])[:4]
        lin["cost"] = float(np.sum(lin["c"] * self.w + lin["mc"]))
        return lin


def smooth(obs, tag_map, K, dist, tag_size, seed, sigma_px, sigma_rot, sigma_trans, huber_px, max_iters, reverse=False):
    """smooth_ref.smooth under the Huber loss -> ((n_frames,) CAM_POSE_DTYPE with n_rejected the soft slots, SMOOTH_RESULT_DTYPE
    record with n_soft, trace); trace: smooth_ref's "posed", "d", "tr", "choice", and "lins": the linearisation of the chain's
    poses and of every trial computed (accepted or not), "P": the camera<-world poses returned, "problem": the Problem"""
    obs = np.asarray(obs)
    pb = Problem(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, huber_px, reverse)
    n = pb.n
    out = np.zeros(n, dtype=CAM_POSE_DTYPE)
    out["T"] = np.eye(4)
    out["seed_slot"] = -1
    out["status"] = SR.FRAME_NOTHING
    res = np.zeros((), dtype=SMOOTH_RESULT_DTYPE)
    cand = SR.candidates(pb, seed)
    posed, d, tr = SR.chain_costs(pb, cand)
    trace = {"posed": posed, "d": d, "tr": tr, "choice": np.zeros(0, dtype=np.int64), "lins": [], "P": None, "problem": pb}
    if not posed:
        res["status"] = SR.NO_POSED_FRAME
        return out, res, trace
    choice = SR.chain_choose(d, tr)
    trace["choice"] = choice
    P, src = [], -1
    for f in range(n):
        if cand[f] is not None:
            src += 1
        k = max(src, 0)
        P.append(cand[posed[k]][choice[k]])
        if cand[f] is not None:
            out["seed_slot"][f] = seed["seed_slot"][f] + SR.FLIPPED * choice[k]
    out["n_tags"] = pb.n_tags
    res["n_frames_data"] = int((pb.n_tags > 0).sum())
    res["n_filled"] = n - len(posed)
    res["n_flipped"] = int(choice.sum())

    lin = pb.linearise(P)
    trace["lins"].append((P, lin))
    corners = 4.0 * float(pb.n_tags.sum())

    def rms(c, k):
        return np.sqrt(c / k) if k > 0 else 0.0

    res["cost_seed"], res["rms_seed_px"] = lin["cost"], rms(float(lin["c"].sum()), corners)
    out["rms_seed_px"] = [rms(c, 4.0 * k) for c, k in zip(lin["c"], pb.n_tags)]
    status, iters = SR.OK, 0
    if not np.isfinite(lin["cost"]):
        status = SR.NON_FINITE
    else:
        lam, solved = SR.LAMBDA0, False
        for _ in range(int(max_iters)):
            iters += 1
            delta = SR.tridiag_solve(*pb.blocks(lin), lam)
            if delta is None:
                lam *= 10
                continue
            solved = True
            Pn = [SR.update(P[f], delta[f]) for f in range(n)]
            ln = pb.linearise(Pn)
            trace["lins"].append((Pn, ln))
            if ln["cost"] < lin["cost"]:
                stop = lin["cost"] - ln["cost"] < SR.REL_STOP * lin["cost"]
                P, lin = Pn, ln
                lam *= 0.1
                if stop:
                    break
            else:
                lam *= 10
        if not solved:
            status = SR.NOT_POSITIVE_DEFINITE
    for f in range(n):
        T = np.eye(4)
        T[:3, :3] = P[f][0].T
        T[:3, 3] = -(P[f][0].T @ P[f][1])
        out["T"][f] = T
    out["rms_px"] = [rms(c, 4.0 * k) for c, k in zip(lin["c"], pb.n_tags)]
    out["n_rejected"] = lin["soft"]
    out["status"] = SR.FRAME_FAILED if status != SR.OK else np.where(pb.n_tags > 0, SR.FRAME_DATA, SR.FRAME_PRIOR)
    res["cost"], res["rms_px"], res["iterations"], res["status"] = lin["cost"], rms(float(lin["c"].sum()), corners), iters, status
    res["n_soft"] = int(lin["soft"].sum())
    trace["P"] = P
    return out, res, trace


def problem_blocks(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px):
    """(problem, camera<-world poses, D, C) of the robust problem relinearised at the poses of a smooth output"""
    pb = Problem(np.asarray(obs), tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, huber_px)
    P = [SR.pose_of_seed(p) for p in poses]
    D, C, _ = pb.blocks(pb.linearise(P))
    return pb, P, D, C


def smooth_cov(obs, tag_map, K, dist, tag_size, poses, result, sigma_px, sigma_rot, sigma_trans, huber_px):
    """smooth_cov_ref.smooth_cov over the weighted normal equations -> (n_frames,) POSE_COV_DTYPE"""
    n = len(poses)
    if int(result["status"]) != SR.OK:
        return SCR.records(n, 0.0, sigma_px, 0, PC.STATUS_NO_POSE)
    pb, P, D, C = problem_blocks(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px)
    dof = 8 * int(pb.n_tags.sum()) - 6
    Sig = SCR.marginals(D, C) if np.all(np.isfinite(D)) and np.all(np.isfinite(C)) else None
    if Sig is None:
        return SCR.records(n, 0.0, sigma_px, dof, PC.STATUS_NOT_PD)
    return SCR.records(n, np.stack([SCR.to_record_convention(Sig[f], P[f][0]) for f in range(n)]), sigma_px, dof, PC.STATUS_OK)


def dense_marginals(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px):
    """the independent second route: (covariances (n, 6, 6) from np.linalg.inv of the assembled weighted matrix, that matrix)"""
    pb, P, D, C = problem_blocks(obs, tag_map, K, dist, tag_size, poses, sigma_px, sigma_rot, sigma_trans, huber_px)
    A = SR.dense(D, C)
    Ai = np.linalg.inv(A)
    out = np.zeros((len(poses), 6, 6))
    for f in range(len(poses)):
        Am = PC.convention_map(P[f][0], P[f][1], True)
        Cf = Am @ Ai[6 * f:6 * f + 6, 6 * f:6 * f + 6] @ Am.T
        out[f] = 0.5 * (Cf + Cf.T)
    return out, A
