"""NumPy statement of the sequence localisation with frame times (asl_smooth_timed_sequences_device / _batch, SmoothBufs.times in
aprilslam_amd/csrc/k_smooth.inc).  It states what differs from tests/smooth_ref.py and takes everything else from there.

Frame f of a sequence is at time times[f] (float64, any unit); sigma_rot and sigma_trans are the random walk's sigmas per
unit of that time.  The pair (f, f + 1), dt_f = times[f + 1] - times[f], has the motion residual

    m_f = (Log(R_D) w_rot, t_D w_trans),    w_rot = (1 / sigma_rot) (1 / sqrt(dt_f)),    w_trans = (1 / sigma_trans) (1 / sqrt(dt_f))

in that operation order, so that dt_f == 1 gives smooth_ref's weights to the bit.  |m_f|^2 is the plain cost divided by dt_f:
what is left of dt_f unit steps of the plain walk when the frames between, which have no data, are marginalised out (the
variances of a random walk add).  The Jacobians Jn = W B, Jp = -W B Ad, the blocks QN, QP, C, gN, gP and |m|^2 use this W per
pair; the assembly, the linear solve, the LM schedule, the corner costs (huber_px included) are smooth_ref's.

Seed chain: the transition cost of a posed frame f from its posed predecessor p is the motion cost at the call's sigmas
divided by times[f] - times[p] (smooth_ref: by f - p).  Candidates, ties, backtracking, fill: smooth_ref's.

Bad times: a time that is not finite, or a dt_f <= 0 (a sequence of one frame needs only a finite time).  Nothing is solved:
the result is that of status 1 (no posed frame) with status 4 (BAD_TIMES), the frames' records those of status 1.

times None is times[f] = f: smooth_ref.smooth, through this driver.

pose_at: the pose at a time between two frames along the prior's own geodesic, a = (t - times[f]) / dt_f:
camera<-world R = Exp(a Log R_D) R_f, t = Exp(a Log R_D) t_f + a t_D -- to first order in the step rotation the walk's
conditional mean between the two poses.  No extrapolation.

Covariance: smooth_cov_ref's recursion and record convention on the timed blocks at the returned poses.
Test infrastructure, as smooth_ref.py is."""
import numpy as np

import localize_ref as LR
import pose_cov_ref as PC
import smooth_cov_ref as SV
import smooth_ref as SR
from aprilslam_amd._lib import CAM_POSE_DTYPE, SMOOTH_RESULT_DTYPE
from smooth_ref import (FLIPPED, FRAME_DATA, FRAME_FAILED, FRAME_NOTHING, FRAME_PRIOR, LAMBDA0, NO_POSED_FRAME, NON_FINITE,
                        NOT_POSITIVE_DEFINITE, OK, REL_STOP, Problem, candidates, chain_choose, log_so3, motion_jacobians, relative,
                        tridiag_solve, update)

BAD_TIMES = 4


def bad_times(times):
    """the status-4 rule of one sequence"""
    t = np.asarray(times, dtype=np.float64)
    return bool((~np.isfinite(t)).any() or (len(t) > 1 and not (np.diff(t) > 0).all()))


class TimedProblem(Problem):
    """smooth_ref.Problem with a time per frame: the per-pair weights in the linearisation"""

    def __init__(self, obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, times, reverse=False, huber_px=0.0):
        super().__init__(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, reverse, huber_px)
        self.times = np.arange(self.n, dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64)

    def pair_weights(self, f):
        isd = 1.0 / np.sqrt(self.times[f + 1] - self.times[f])
        return (1.0 / self.sr) * isd, (1.0 / self.st) * isd

    def linearise(self, P):
        """smooth_ref's per-frame terms; every pair's motion blocks again with the pair's own weights"""
        lin = super().linearise(P)
        for f in range(self.n - 1):
            wr, wt = self.pair_weights(f)
            RD, tD = relative(P[f], P[f + 1])
            m = np.concatenate([log_so3(RD) * wr, tD * wt])
            Jn, Jp = motion_jacobians(RD, tD, 1.0, 1.0)      # (B, -(B Ad)): a weight of 1.0 changes no bit
            w = np.array([wr] * 3 + [wt] * 3)
            Jn, Jp = w[:, None] * Jn, w[:, None] * Jp        # w (-(B Ad)) = -(w (B Ad)) to the bit
            lin["mc"][f] = m @ m
            lin["QN"][f], lin["QP"][f], lin["C"][f] = Jp.T @ Jp, Jn.T @ Jn, Jn.T @ Jp
            lin["gN"][f], lin["gP"][f] = Jp.T @ m, Jn.T @ m
        lin["cost"] = float(np.sum(lin["c"] * self.w + lin["mc"]))
        return lin


def chain_costs(pb, cand):
    """smooth_ref.chain_costs with the transition divided by the time between the two posed frames"""
    posed = [f for f in range(pb.n) if cand[f] is not None]
    d = np.zeros((len(posed), 2))
    tr = np.zeros((len(posed), 2, 2))
    for k, f in enumerate(posed):
        for b in (0, 1):
            d[k, b] = pb.data_cost(f, cand[f][b]) * pb.w
            for a in (0, 1):
                if k:
                    p = posed[k - 1]
                    tr[k, a, b] = pb.motion_cost(cand[p][a], cand[f][b]) / (pb.times[f] - pb.times[p])
    return posed, d, tr


def smooth(obs, tag_map, K, dist, tag_size, seed, times, sigma_px, sigma_rot, sigma_trans, max_iters, reverse=False, huber_px=0.0):
    """smooth_ref.smooth with times (n_frames,) or None -> the same three: ((n_frames,) CAM_POSE_DTYPE, SMOOTH_RESULT_DTYPE
    record, trace)"""
    obs = np.asarray(obs)
    n = len(obs)
    out = np.zeros(n, dtype=CAM_POSE_DTYPE)
    out["T"] = np.eye(4)
    out["seed_slot"] = -1
    out["status"] = FRAME_NOTHING
    res = np.zeros((), dtype=SMOOTH_RESULT_DTYPE)
    trace = {"posed": [], "d": np.zeros((0, 2)), "tr": np.zeros((0, 2, 2)), "choice": np.zeros(0, dtype=np.int64), "lins": [], "P": None,
             "problem": None}
    if times is not None and bad_times(times):
        res["status"] = BAD_TIMES
        return out, res, trace
    pb = TimedProblem(obs, tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, times, reverse, huber_px)
    cand = candidates(pb, seed)
    posed, d, tr = chain_costs(pb, cand)
    trace.update(posed=posed, d=d, tr=tr, problem=pb)
    if not posed:
        res["status"] = NO_POSED_FRAME
        return out, res, trace
    choice = chain_choose(d, tr)
    trace["choice"] = choice
    P, src = [], -1
    for f in range(n):
        if cand[f] is not None:
            src += 1
        k = max(src, 0)
        P.append(cand[posed[k]][choice[k]])
        if cand[f] is not None:
            out["seed_slot"][f] = seed["seed_slot"][f] + FLIPPED * choice[k]
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
    status, iters = OK, 0
    if not np.isfinite(lin["cost"]):
        status = NON_FINITE
    else:
        lam, solved = LAMBDA0, False
        for _ in range(int(max_iters)):
            iters += 1
            delta = tridiag_solve(*pb.blocks(lin), lam)
            if delta is None:
                lam *= 10
                continue
            solved = True
            Pn = [update(P[f], delta[f]) for f in range(n)]
            ln = pb.linearise(Pn)
            trace["lins"].append((Pn, ln))
            if ln["cost"] < lin["cost"]:
                stop = lin["cost"] - ln["cost"] < REL_STOP * lin["cost"]
                P, lin = Pn, ln
                lam *= 0.1
                if stop:
                    break
            else:
                lam *= 10
        if not solved:
            status = NOT_POSITIVE_DEFINITE
    for f in range(n):
        T = np.eye(4)
        T[:3, :3] = P[f][0].T
        T[:3, 3] = -(P[f][0].T @ P[f][1])
        out["T"][f] = T
    out["rms_px"] = [rms(c, 4.0 * k) for c, k in zip(lin["c"], pb.n_tags)]
    out["n_rejected"] = lin["soft"]
    out["status"] = FRAME_FAILED if status != OK else np.where(pb.n_tags > 0, FRAME_DATA, FRAME_PRIOR)
    res["cost"], res["rms_px"], res["iterations"], res["status"] = lin["cost"], rms(float(lin["c"].sum()), corners), iters, status
    res["n_soft"] = int(lin["soft"].sum())
    trace["P"] = P
    return out, res, trace


def smooth_sequences(obs, seq_start, tag_map, K, dist, tag_size, seed, times, sigma_px, sigma_rot, sigma_trans, max_iters, huber_px=0.0):
    """a call of several sequences: each alone on its own frames and times[a0:a1] -> ((n_frames,) poses, (n_seq,) results)"""
    obs = np.asarray(obs)
    out, res = np.zeros(len(obs), dtype=CAM_POSE_DTYPE), np.zeros(len(seq_start) - 1, dtype=SMOOTH_RESULT_DTYPE)
    for k, (a, b) in enumerate(zip(seq_start[:-1], seq_start[1:])):
        out[a:b], res[k], _ = smooth(obs[a:b], tag_map, K, dist, tag_size, seed[a:b], None if times is None else times[a:b], sigma_px,
                                     sigma_rot, sigma_trans, max_iters, huber_px=huber_px)
    return out, res


def pose_at(T, times, t):
    """(4, 4) world<-camera at time t of the world<-camera poses T (n, 4, 4) at times (None: the frame indices)"""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    times = np.arange(len(T), dtype=np.float64) if times is None else np.asarray(times, dtype=np.float64)
    if not (times[0] <= t <= times[-1]):
        raise ValueError("no extrapolation")
    f = int(np.searchsorted(times, t, side="right")) - 1
    if f == len(T) - 1 or t == times[f]:
        return T[f].copy()
    Pa, Pb = SR.pose_of_seed({"T": T[f]}), SR.pose_of_seed({"T": T[f + 1]})
    a = (t - times[f]) / (times[f + 1] - times[f])
    RD, tD = relative(Pa, Pb)
    E = LR.rodrigues(a * log_so3(RD))
    R, tv = E @ Pa[0], E @ Pa[1] + a * tD
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R.T, -(R.T @ tv)
    return out


def problem_blocks(obs, tag_map, K, dist, tag_size, poses, times, sigma_px, sigma_rot, sigma_trans, huber_px=0.0):
    """smooth_cov_ref.problem_blocks on the timed problem: (problem, camera<-world poses, D, C) at the poses of an output"""
    pb = TimedProblem(np.asarray(obs), tag_map, K, dist, tag_size, sigma_px, sigma_rot, sigma_trans, times, huber_px=huber_px)
    P = [SR.pose_of_seed(p) for p in poses]
    D, C, _ = pb.blocks(pb.linearise(P))
    return pb, P, D, C


def smooth_cov(obs, tag_map, K, dist, tag_size, poses, result, times, sigma_px, sigma_rot, sigma_trans, huber_px=0.0):
    """smooth_cov_ref.smooth_cov of a timed output -> ((n_frames,) POSE_COV_DTYPE, the assembled matrix A or None)"""
    n = len(poses)
    if int(result["status"]) != OK:
        return SV.records(n, 0.0, sigma_px, 0, PC.STATUS_NO_POSE), None
    pb, P, D, C = problem_blocks(obs, tag_map, K, dist, tag_size, poses, times, sigma_px, sigma_rot, sigma_trans, huber_px)
    dof = 8 * int(pb.n_tags.sum()) - 6
    Sig = SV.marginals(D, C) if np.all(np.isfinite(D)) and np.all(np.isfinite(C)) else None
    if Sig is None:
        return SV.records(n, 0.0, sigma_px, dof, PC.STATUS_NOT_PD), None
    return SV.records(n, np.stack([SV.to_record_convention(Sig[f], P[f][0]) for f in range(n)]), sigma_px, dof, PC.STATUS_OK), SR.dense(D, C)
