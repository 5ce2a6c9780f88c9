// Rig mounting calibration (asl_calibrate_rig_frames_device / asl_calibrate_rig_batch): the mountings E_c = camera_c<-rig of a
// rig's cameras, refined jointly with one pose rig<-world per frame against a known tag map, float64 throughout;
// tests/rig_calib_ref.py is the NumPy statement of the same computation.  The rig model is k_rig.inc's (rig_corner, LocRig),
// the problem has the arrow shape of k_calib.inc: 6 shared parameters per solved camera, one 6-parameter pose per frame that
// the frame eliminates (Schur complement), a small dense reduced system (<= 42 x 42).
//   k_localize_rig   the seed: every frame under the initial mountings, the gate off, written to the poses as they are
//   k_rigcal_init    per frame (one wavefront): the frame's camera mask and taking-part slots; block 0: the camera table
//   k_rigcal_connect one workgroup: the cameras connected to camera 0 through frames that two or more cameras see (reach),
//                    the list of used frames, the solved cameras, the counts, lambda0
//   k_rigcal_first   per used frame: rig<-world of its seed, its normal equations there
//   k_rigcal_start   one workgroup: the initial cost
//   then max_iters times (joint Levenberg-Marquardt):
//   k_rigcal_schur   per used frame: Cholesky of its damped 6x6 pose block U, U^-1 W, U^-1 g_pose and its share of the
//                    reduced system blockdiag(V) - W^T U^-1 W, g - W^T U^-1 g_pose
//   k_rigcal_solve   one workgroup: the shares summed, Cholesky of the reduced system -> the mountings' step, the trial mountings
//   k_rigcal_step    per used frame: its pose step (back-substitution), the trial pose and its normal equations there
//   k_rigcal_decide  one workgroup: trial cost against the current one, lambda x0.1 / x10, accept (flip the buffers), stop
//   and once more k_rigcal_schur undamped, k_rigcal_finish (covariances from the reduced system's inverse, the records).
// As in k_calib.inc lambda, the accepted state (cur: which of the two pose / normal-equation / camera-table buffers is
// current) and the stop flag live in device memory, the whole solve is one submission, and every kernel returns at once
// after the stop.  Sums over corners are butterfly sums, sums over frames cal_list_sum's: no atomics, the same bytes on
// every run.  Latency-bound: ~4 dependent launches per trial.
//
// The sweeps of k_rigcal_connect: the statement sweeps the frames in order and lets a frame see what earlier frames of the
// same sweep added; here every frame of a sweep sees reach as it was when the sweep began.  Either way a sweep that adds
// nothing ends the growth and one that adds something adds a camera, so after n_cams - 1 sweeps both hold the cameras
// connected to camera 0, the same set.

struct RigCalResultRec {  // == asl_rig_calib_result, 176 bytes
    double rms_px, rms_init_px, sigma_px;
    int32_t n_frames_used, n_corners, iterations, status, n_solved, reserved;
    int32_t cam_status[16], cam_frames[16];
};

#define RC_MAX_CAMS 8
#define RC_MAX_P (6 * (RC_MAX_CAMS - 1))                 // unknowns of the reduced system
#define RC_MAX_SB (RC_MAX_P * (RC_MAX_P + 1) / 2 + RC_MAX_P)  // 945: S packed, then b
#define RC_SB_LDS ((RC_MAX_SB + 63) / 64 * 64)           // cal_list_sum's out
#define RC_CAM 63   // doubles of a solved camera in a frame's normal equations: W (6 x 6, row: pose, column: mounting) 36, V packed 21, g 6
#define RC_HS0 28   // before them: U packed 21, g_pose 6, the cost
#define RC_FR 5     // ints per frame: seed status, camera mask, taking-part slots, Schur ok, used

// doubles per frame of the normal equations, of the reduced system's share and of the back-substitution for ns solved cameras
__host__ __device__ constexpr int rc_hs(int ns) { return RC_HS0 + RC_CAM * ns; }
__host__ __device__ constexpr int rc_sb(int ns) { return 6 * ns * (6 * ns + 1) / 2 + 6 * ns; }
__host__ __device__ constexpr int rc_bk(int ns) { return 6 + 36 * ns; }   // U^-1 g_pose, then U^-1 W column by column

struct RigCalState {
    double dm[RC_MAX_P];  // the trial's step of the mountings
    double lambda, cost, cost0;
    int cur, done, solve_ok, status, iterations, n_used, n_corners, n_solved, reach, count;
    int col[RC_MAX_CAMS];         // camera -> its place among the solved ones, -1 if it is not solved
    int cam[RC_MAX_CAMS];         // the solved cameras in camera order
    int cam_frames[RC_MAX_CAMS];  // the used frames with the camera in their mask
};

struct RigCalArgs {
    const ObsRec *obs;
    const MapTagRec *map;
    const RigCamRec *rig;
    RigCamRec *rig_out;
    RigCalState *st;
    int *list, *fr;
    double *camtab, *pose, *H, *SB, *back;  // camtab: 2 x n_cams x RIG_CAM_DOUBLES; pose, H: 2 x n_frames x (12, hs)
    RigCalResultRec *res;
    PoseCovRec *cov;
    CamPoseRec *out;
    double half, sigma_px;
    unsigned int magic;
    int n_cams, n_frames, max_tags, n_ids, max_iters, hs, sbs, bks;
};

// The frame's camera table (buffer buf) and its gather into LDS; returns the slot model over them
__device__ __forceinline__ LocRig rc_frame(const RigCalArgs &a, int f, int buf, double *s_dyn, LocLds &L, int lane)
{
    const double *tab = a.camtab + (size_t)buf * a.n_cams * RIG_CAM_DOUBLES;
    for (int i = lane; i < RIG_CAM_DOUBLES * a.n_cams; i += ASL_WAVE) s_dyn[i] = tab[i];
    const LocRig m{s_dyn, a.obs, a.magic, a.n_cams, a.max_tags, a.n_frames, f};
    L = loc_lds(s_dyn + RIG_CAM_DOUBLES * a.n_cams, m.nslots());
    loc_gather([&](int s) { return m.rec(s); }, m.nslots(), a.map, a.n_ids, a.half, [](int) { return false; }, L, lane);
    return m;
}

// Entries [LO, HI) of a solved camera's block (W 36, V packed 21, g 6), summed over the corners [k0, k1) of that camera and
// written to Hc.  Two chunks keep the accumulators in registers; the corner's rows are recomputed per chunk (cal_chunk).
template <int LO, int HI>
__device__ __forceinline__ void rc_cam_chunk(const double *cl, const double *R, const double *t, const LocLds &L, int k0, int k1, int lane, double *Hc)
{
    double acc[HI - LO];
#pragma unroll
    for (int i = 0; i < HI - LO; i++) acc[i] = 0;
    for (int k = k0 + lane; k < k1; k += ASL_WAVE) {
        if (L.state[k >> 2] != 1) continue;
        double rw[RIG_ROWS];
#pragma unroll
        for (int i = 0; i < RIG_ROWS; i++) rw[i] = 0;  // a corner behind the camera has no rows
        rig_corner<true, false, true>(cl, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], rw);
        const double *J0 = rw, *J1 = rw + 6, *M0 = rw + 12, *M1 = rw + 18;
#pragma unroll
        for (int p = 0; p < 6; p++) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int iw = 6 * p + q, iv = 36 + TRI(p, q);
                if (iw >= LO && iw < HI) acc[iw - LO] += J0[p] * M0[q] + J1[p] * M1[q];
                if (q <= p && iv >= LO && iv < HI) acc[iv - LO] += M0[p] * M0[q] + M1[p] * M1[q];
            }
            if (57 + p >= LO && 57 + p < HI) acc[57 + p - LO] += M0[p] * rw[24] + M1[p] * rw[25];
        }
    }
#pragma unroll
    for (int i = 0; i < HI - LO; i++) {
        const double v = butterfly_sum<64>(acc[i]);
        if (lane == ((LO + i) & (ASL_WAVE - 1))) Hc[LO + i] = v;
    }
}

// The frame's normal equations at the rig pose (R, t) under the camera table of m, into Hf: U, g_pose and the cost by one
// pass over all corners (loc_pass), then the block of every solved camera, zeros for one that is not in the frame's mask
__device__ __forceinline__ void rc_linearise(const RigCalArgs &a, const LocRig &m, const LocLds &L, const double *R, const double *t, int mask,
                                             int lane, double *Hf)
{
    double ne[27];
    const double cost = loc_pass<true>(m, R, t, L, lane, ne);
#pragma unroll
    for (int i = 0; i < 27; i++)
        if (lane == i) Hf[i] = ne[i];
    if (lane == 27) Hf[27] = cost;
    const int ns = a.st->n_solved;
    for (int j = 0; j < ns; j++) {
        const int c = a.st->cam[j];
        double *Hc = Hf + RC_HS0 + RC_CAM * j;
        if (!((mask >> c) & 1)) {
            if (lane < RC_CAM) Hc[lane] = 0.0;
            continue;
        }
        const double *cl = m.cams + RIG_CAM_DOUBLES * c;
        rc_cam_chunk<0, 36>(cl, R, t, L, 4 * c * a.max_tags, 4 * (c + 1) * a.max_tags, lane, Hc);
        rc_cam_chunk<36, RC_CAM>(cl, R, t, L, 4 * c * a.max_tags, 4 * (c + 1) * a.max_tags, lane, Hc);
    }
}

// Cholesky factor of the packed n x n matrix A in LDS, in place, by the whole workgroup: column by column, the pivot, the
// column, then the update of what lies to its right -- every entry meets its subtractions in the order of cal_chol.
// False (every thread) if A is not positive definite; s_bad: an int of LDS.
__device__ __forceinline__ bool rc_chol_wg(double *A, int n, int *s_bad)
{
    const int tid = threadIdx.x;
    if (tid == 0) *s_bad = 0;
    for (int j = 0; j < n; j++) {
        __syncthreads();
        if (tid == 0) {
            const double s = A[TRI(j, j)];
            if (!(s > 0)) *s_bad = 1;
            A[TRI(j, j)] = sqrt(s);
        }
        __syncthreads();
        const double piv = A[TRI(j, j)];
        if (tid > j && tid < n) A[TRI(tid, j)] = A[TRI(tid, j)] / piv;
        __syncthreads();
        for (int p = tid; p < n * n; p += CAL_WG) {
            const int i = p / n, k = p - i * n;
            if (k > j && i >= k) A[TRI(i, k)] -= A[TRI(i, j)] * A[TRI(k, j)];
        }
    }
    __syncthreads();
    return !*s_bad;
}

// x <- A^-1 x with A's Cholesky factor (packed, LDS), by one thread
__device__ __forceinline__ void rc_chol_subst(const double *A, double *x, int n)
{
    for (int i = 0; i < n; i++) {
        double s = x[i];
        for (int k = 0; k < i; k++) s -= A[TRI(i, k)] * x[k];
        x[i] = s / A[TRI(i, i)];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i];
        for (int k = i + 1; k < n; k++) s -= A[TRI(k, i)] * x[k];
        x[i] = s / A[TRI(i, i)];
    }
}

// ---- per frame: the camera mask and the taking-part slots; block 0: both camera tables from the rig as given
__global__ void __launch_bounds__(64) k_rigcal_init(RigCalArgs a)
{
    const int f = blockIdx.x, lane = threadIdx.x, n = a.n_cams * a.max_tags;
    if (f == 0) {
        rig_fill_cams(a.camtab, a.rig, a.n_cams, lane);
        rig_fill_cams(a.camtab + a.n_cams * RIG_CAM_DOUBLES, a.rig, a.n_cams, lane);
    }
    unsigned int mask = 0;
    int npart = 0;
    for (int g = lane; g < n; g += ASL_WAVE) {
        const int c = rig_cam_of(g, a.magic);
        const ObsRec *r = a.obs + ((size_t)c * a.n_frames + f) * a.max_tags + (g - c * a.max_tags);
        const int id = r->id;
        double hs = a.half;
        if (!((r->flags & 1) && id >= 0 && id < a.n_ids && map_tag_half(a.map[id], hs))) continue;
        npart++;
        mask |= 1u << c;
    }
    mask |= lane_xor32<1>(mask); mask |= lane_xor32<2>(mask); mask |= lane_xor32<4>(mask);
    mask |= lane_xor32<8>(mask); mask |= lane_xor32<16>(mask); mask |= lane_xor32<32>(mask);
    npart = butterfly_sum<64>(npart);
    if (lane == 0) {
        int *fr = a.fr + RC_FR * f;
        fr[0] = a.out[f].status; fr[1] = (int)mask; fr[2] = npart; fr[3] = 0; fr[4] = 0;
    }
}

// ---- one workgroup: reach, the used frames, the solved cameras, the counts
__global__ void __launch_bounds__(CAL_WG) k_rigcal_connect(RigCalArgs a)
{
    __shared__ int s_cnt[CAL_WG];
    __shared__ int s_reach;
    RigCalState *st = a.st;
    const int tid = threadIdx.x;
    if (tid == 0) s_reach = 1;
    __syncthreads();
    auto joins = [&](int f) { return a.fr[RC_FR * f] == 0 && __popc((unsigned int)a.fr[RC_FR * f + 1]) >= 2; };
    for (int sweep = 0; sweep < a.n_cams - 1; sweep++) {
        const int reach = s_reach;
        int add = 0;
        for (int f = tid; f < a.n_frames; f += CAL_WG)
            if (joins(f) && (a.fr[RC_FR * f + 1] & reach)) add |= a.fr[RC_FR * f + 1];
        s_cnt[tid] = add;
        __syncthreads();
        if (tid == 0) {
            int r = reach;
            for (int i = 0; i < CAL_WG; i++) r |= s_cnt[i];
            s_reach = r;
        }
        __syncthreads();
    }
    const int reach = s_reach;
    auto used = [&](int f) { return joins(f) && (a.fr[RC_FR * f + 1] & ~reach) == 0; };
    const int n = cal_make_list_of(a.n_frames, used, a.list, s_cnt, &st->count);
    for (int k = tid; k < n; k += CAL_WG) a.fr[RC_FR * a.list[k] + 4] = 1;
    // taking-part slots and, per camera, frames over the list (integers: exact in any order)
    int slots = 0;
    for (int k = tid; k < n; k += CAL_WG) slots += a.fr[RC_FR * a.list[k] + 2];
    s_cnt[tid] = slots;
    __syncthreads();
    if (tid == 0) {
        int corners = 0;
        for (int i = 0; i < CAL_WG; i++) corners += s_cnt[i];
        st->n_corners = 4 * corners;
    }
    __syncthreads();
    // per camera: every thread counts its share of the list, the waves sum theirs (butterfly), camera c's thread the 16 waves
    int cf[RC_MAX_CAMS];
#pragma unroll
    for (int c = 0; c < RC_MAX_CAMS; c++) cf[c] = 0;
    for (int k = tid; k < n; k += CAL_WG) {
        const int m = a.fr[RC_FR * a.list[k] + 1];
#pragma unroll
        for (int c = 0; c < RC_MAX_CAMS; c++) cf[c] += (m >> c) & 1;
    }
#pragma unroll
    for (int c = 0; c < RC_MAX_CAMS; c++) {
        const int w = butterfly_sum<64>(cf[c]);
        if ((tid & 63) == 0) s_cnt[c * CAL_CHUNKS + (tid >> 6)] = w;
    }
    __syncthreads();
    if (tid < RC_MAX_CAMS) {
        int total = 0;
        for (int j = 0; j < CAL_CHUNKS; j++) total += s_cnt[tid * CAL_CHUNKS + j];
        st->cam_frames[tid] = tid < a.n_cams ? total : 0;
    }
    if (tid == 0) {
        int ns = 0;
        for (int c = 0; c < RC_MAX_CAMS; c++) {
            const bool solved = c > 0 && c < a.n_cams && ((reach >> c) & 1);
            st->col[c] = solved ? ns : -1;
            if (solved) st->cam[ns++] = c;
        }
        for (int j = ns; j < RC_MAX_CAMS; j++) st->cam[j] = 0;
        for (int i = 0; i < RC_MAX_P; i++) st->dm[i] = 0;
        const long long dof = 2 * (long long)st->n_corners - 6 * (long long)n - 6 * ns;
        const int status = (ns == 0 || dof <= 0) ? 1 : 0;
        st->lambda = 1e-3; st->cost = 0; st->cost0 = 0;
        st->cur = 0; st->done = status != 0; st->solve_ok = 0; st->status = status; st->iterations = 0;
        st->n_used = n; st->n_solved = ns; st->reach = reach;
    }
}

// ---- per used frame: rig<-world of the seed's world<-rig, the frame's normal equations there
__global__ void __launch_bounds__(64) k_rigcal_first(RigCalArgs a)
{
    extern __shared__ double s_dyn[];
    const RigCalState *st = a.st;
    const int lane = threadIdx.x;
    if (st->status != 0 || (int)blockIdx.x >= st->n_used) return;
    const int f = a.list[blockIdx.x];
    const double *T = a.out[f].T;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) R[3 * i + k] = T[4 * k + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = -(R[3 * i] * T[3] + R[3 * i + 1] * T[7] + R[3 * i + 2] * T[11]);
    double *P = a.pose + (size_t)12 * f;  // buffer 0: cur = 0 at the start
    if (lane < 9) P[lane] = T[4 * (lane % 3) + lane / 3];
    if (lane == 0) { P[9] = t[0]; P[10] = t[1]; P[11] = t[2]; }
    LocLds L;
    const LocRig m = rc_frame(a, f, 0, s_dyn, L, lane);
    rc_linearise(a, m, L, R, t, a.fr[RC_FR * f + 1], lane, a.H + (size_t)a.hs * f);
}

// ---- one workgroup: the initial cost
__global__ void __launch_bounds__(CAL_WG) k_rigcal_start(RigCalArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64];
    RigCalState *st = a.st;
    if (st->status != 0) return;
    cal_list_sum(a.H + 27, a.hs, 1, a.list, st->n_used, s_part, s_sum);
    if (threadIdx.x == 0) { st->cost = s_sum[0]; st->cost0 = s_sum[0]; }
}

// ---- per used frame: the pose block eliminated; final = 1: undamped, at the solution (for the covariances)
__global__ void __launch_bounds__(64) k_rigcal_schur(RigCalArgs a, int final)
{
    __shared__ double s_H[rc_hs(RC_MAX_CAMS - 1)], s_UW[6 * RC_MAX_P], s_Ug[6];
    const RigCalState *st = a.st;
    const int lane = threadIdx.x;
    if (st->status != 0 || (!final && st->done) || (int)blockIdx.x >= st->n_used) return;
    const int f = a.list[blockIdx.x], cur = st->cur, ns = st->n_solved, np = 6 * ns, hs = rc_hs(ns);
    const double lam1 = final ? 1.0 : 1.0 + st->lambda;
    const double *Hf = a.H + ((size_t)cur * a.n_frames + f) * a.hs;
    for (int i = lane; i < hs; i += ASL_WAVE) s_H[i] = Hf[i];
    __syncthreads();
    double U[21];
#pragma unroll
    for (int i = 0; i < 21; i++) U[i] = s_H[i];
#pragma unroll
    for (int i = 0; i < 6; i++) U[TRI(i, i)] *= lam1;
    // Cholesky of U (every lane, identical), then lane i < np: U^-1 W[:, i]; lane np: U^-1 g_pose
    double b[6] = {0, 0, 0, 0, 0, 0};
    if (lane < np) {
        const double *Wc = s_H + RC_HS0 + RC_CAM * (lane / 6) + lane % 6;
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = Wc[6 * k];
    } else if (lane == np) {
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = s_H[21 + k];
    }
    const bool ok = chol6_solve_tri_dev(U, b);
    if (lane < np) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_UW[6 * lane + k] = b[k];
    } else if (lane == np) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_Ug[k] = b[k];
    }
    __syncthreads();
    double *SB = a.SB + (size_t)a.sbs * f, *BK = a.back + (size_t)a.bks * f;
    // row i of the share by the lanes j <= i: S_ij = V_ij - W_i . (U^-1 W)_j, V only inside a camera's own block
    for (int i = 0; i < np; i++) {
        if (lane > i) continue;
        const int j = lane, ci = i / 6, pi = i % 6;
        const double *Hc = s_H + RC_HS0 + RC_CAM * ci;
        double v = 0;
        if (j / 6 == ci) v = Hc[36 + TRI(pi, j % 6)];
        if (i == j) v *= lam1;
        for (int k = 0; k < 6; k++) v -= Hc[6 * k + pi] * s_UW[6 * j + k];
        SB[TRI(i, j)] = v;
    }
    if (lane < np) {  // b_i = g_i - W_i . U^-1 g_pose
        const double *Hc = s_H + RC_HS0 + RC_CAM * (lane / 6);
        double v = Hc[57 + lane % 6];
        for (int k = 0; k < 6; k++) v -= Hc[6 * k + lane % 6] * s_Ug[k];
        SB[np * (np + 1) / 2 + lane] = v;
    }
    if (lane < 6) BK[lane] = s_Ug[lane];
    for (int e = lane; e < 6 * np; e += ASL_WAVE) BK[6 + e] = s_UW[e];
    if (lane == 0) a.fr[RC_FR * f + 3] = ok ? 1 : 0;
}

// the frames' shares summed into s_S (LDS, RC_SB_LDS doubles), and whether every frame's own Cholesky held (every thread)
__device__ __forceinline__ bool rc_reduced(const RigCalArgs &a, int n, int np, double *s_part, double *s_S, int *s_bad)
{
    if (threadIdx.x == 0) *s_bad = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += CAL_WG)
        if (a.fr[RC_FR * a.list[k] + 3] == 0) *s_bad = 1;
    cal_list_sum(a.SB, a.sbs, np * (np + 1) / 2 + np, a.list, n, s_part, s_S);
    const bool bad = *s_bad != 0;
    __syncthreads();
    return !bad;
}

// ---- one workgroup: the reduced system, the mountings' step, the trial mountings
__global__ void __launch_bounds__(CAL_WG) k_rigcal_solve(RigCalArgs a)
{
    __shared__ double s_part[CAL_WG], s_S[RC_SB_LDS];
    __shared__ int s_bad;
    RigCalState *st = a.st;
    if (st->status != 0 || st->done) return;
    const int n = st->n_used, ns = st->n_solved, np = 6 * ns, cur = st->cur;
    bool ok = rc_reduced(a, n, np, s_part, s_S, &s_bad);
    ok = rc_chol_wg(s_S, np, &s_bad) && ok;
    double *d = s_part;
    if (threadIdx.x == 0) {
        const double *bb = s_S + np * (np + 1) / 2;
        for (int i = 0; i < np; i++) d[i] = -bb[i];
        if (ok) rc_chol_subst(s_S, d, np);
        for (int i = 0; i < np; i++) st->dm[i] = ok ? d[i] : 0.0;
        st->solve_ok = ok;
    }
    __syncthreads();
    if (ok && (int)threadIdx.x < ns) {  // the trial mounting of solved camera j: (Rod(w) Re, Rod(w) te + v)
        const int j = threadIdx.x, c = st->cam[j];
        const double *E0 = a.camtab + ((size_t)cur * a.n_cams + c) * RIG_CAM_DOUBLES + 9;
        double *E1 = a.camtab + ((size_t)(1 - cur) * a.n_cams + c) * RIG_CAM_DOUBLES + 9;
        double w[3], Re[9], dR[9], Rn[9];
        for (int i = 0; i < 3; i++) w[i] = d[6 * j + i];
        for (int i = 0; i < 9; i++) Re[i] = E0[i];
        rodrigues_dev(w, dR);
        mat3_mul_dev(dR, Re, Rn);
        for (int i = 0; i < 9; i++) E1[i] = Rn[i];
        for (int r = 0; r < 3; r++) E1[9 + r] = dR[3 * r] * E0[9] + dR[3 * r + 1] * E0[10] + dR[3 * r + 2] * E0[11] + d[6 * j + 3 + r];
    }
}

// ---- per used frame: the pose step, the trial pose and its normal equations under the trial mountings
__global__ void __launch_bounds__(64) k_rigcal_step(RigCalArgs a)
{
    extern __shared__ double s_dyn[];
    const RigCalState *st = a.st;
    const int lane = threadIdx.x;
    if (st->status != 0 || st->done || !st->solve_ok || (int)blockIdx.x >= st->n_used) return;
    const int f = a.list[blockIdx.x], cur = st->cur, np = 6 * st->n_solved;
    const double *BK = a.back + (size_t)a.bks * f, *P = a.pose + ((size_t)cur * a.n_frames + f) * 12;
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = 0;
        for (int j = 0; j < np; j++) v += BK[6 + 6 * j + i] * st->dm[j];
        d[i] = -(BK[i] + v);
    }
    double R0[9], t0[3], dR[9], R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R0[i] = P[i];
    t0[0] = P[9]; t0[1] = P[10]; t0[2] = P[11];
    rodrigues_dev(d, dR);
    mat3_mul_dev(dR, R0, R);
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = dR[3 * r] * t0[0] + dR[3 * r + 1] * t0[1] + dR[3 * r + 2] * t0[2] + d[3 + r];
    double *Pn = a.pose + ((size_t)(1 - cur) * a.n_frames + f) * 12;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) Pn[i] = R[i];
        Pn[9] = t[0]; Pn[10] = t[1]; Pn[11] = t[2];
    }
    LocLds L;
    const LocRig m = rc_frame(a, f, 1 - cur, s_dyn, L, lane);
    rc_linearise(a, m, L, R, t, a.fr[RC_FR * f + 1], lane, a.H + ((size_t)(1 - cur) * a.n_frames + f) * a.hs);
}

// ---- one workgroup: accept or reject the trial (k_calib_decide's rule)
__global__ void __launch_bounds__(CAL_WG) k_rigcal_decide(RigCalArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64];
    RigCalState *st = a.st;
    if (st->status != 0 || st->done) return;
    const int cur = st->cur;
    const bool solved = st->solve_ok;
    if (solved) cal_list_sum(a.H + ((size_t)(1 - cur) * a.n_frames) * a.hs + 27, a.hs, 1, a.list, st->n_used, s_part, s_sum);
    if (threadIdx.x == 0) {
        st->iterations += 1;
        const double cost = st->cost;
        if (solved && s_sum[0] < cost) {
            const double cn = s_sum[0];
            st->cost = cn;
            st->cur = 1 - cur;
            st->lambda *= 0.1;
            if (cost - cn < 1e-12 * cost) st->done = 1;
        } else
            st->lambda *= 10;
        if (st->iterations >= a.max_iters) st->done = 1;
    }
    // an accepted trial becomes the current table; the other buffer's solved mountings are rewritten by the next solve
}

// ---- one workgroup: the covariances from the undamped reduced system, the rig, the result and the per-frame records
__global__ void __launch_bounds__(CAL_WG) k_rigcal_finish(RigCalArgs a)
{
    __shared__ double s_part[CAL_WG], s_S[RC_SB_LDS], s_x[RC_MAX_P * RC_MAX_P];
    __shared__ int s_bad;
    RigCalState *st = a.st;
    const int tid = threadIdx.x, cur = st->cur, ns = st->n_solved, np = 6 * ns, n = st->n_used;
    const double *tab = a.camtab + (size_t)cur * a.n_cams * RIG_CAM_DOUBLES;
    int status = st->status;
    if (status == 0) {
        bool fin = isfinite(st->cost);
        for (int j = 0; j < ns; j++)
            for (int i = 9; i < RIG_CAM_DOUBLES; i++) fin = fin && isfinite(tab[RIG_CAM_DOUBLES * st->cam[j] + i]);
        if (!fin) status = 3;
    }
    if (status == 0) {  // uniform: every thread read the same state
        bool ok = rc_reduced(a, n, np, s_part, s_S, &s_bad);
        ok = rc_chol_wg(s_S, np, &s_bad) && ok;
        if (!ok) status = 3;
    }
    const long long dof = 2 * (long long)st->n_corners - 6 * (long long)n - np;
    double sig = a.sigma_px;
    const double s2 = status == 0 ? pose_cov_sigma2(a.sigma_px, st->cost, (int)dof, &sig) : 0.0;
    if (status == 0) {
        if (tid < np) {  // column tid of S^-1 from the factor
            double *x = s_x + RC_MAX_P * tid;
            for (int k = 0; k < np; k++) x[k] = k == tid ? 1.0 : 0.0;
            rc_chol_subst(s_S, x, np);
        }
        __syncthreads();
    }
    if (tid < a.n_cams) {  // camera tid: its covariance and its record (rig_out may be rig: read, then write)
        const int c = tid, j = st->col[c];
        const bool solved = status == 0 && j >= 0;
        PoseCovRec *oc = a.cov + c;
        if (solved) {
            // C_(w,v): the camera's block of S^-1, its lower triangle; (r, d) = A (w, v), A = [I 0; -[te]x I]
            const double *te = tab + RIG_CAM_DOUBLES * c + 18;
            double A[36], C[36];
            for (int i = 0; i < 36; i++) A[i] = (i % 7 == 0) ? 1.0 : 0.0;
            A[6 * 3 + 1] = te[2]; A[6 * 3 + 2] = -te[1];
            A[6 * 4 + 0] = -te[2]; A[6 * 4 + 2] = te[0];
            A[6 * 5 + 0] = te[1]; A[6 * 5 + 1] = -te[0];
            for (int r = 0; r < 6; r++)
                for (int k = 0; k <= r; k++) {
                    const double v = s_x[RC_MAX_P * (6 * j + k) + 6 * j + r];
                    C[6 * r + k] = v;
                    C[6 * k + r] = v;
                }
            for (int r = 0; r < 6; r++)
                for (int k = 0; k <= r; k++) {
                    double v = 0;
                    for (int p = 0; p < 6; p++) {
                        double w = 0;
                        for (int q = 0; q < 6; q++) w += C[6 * p + q] * A[6 * k + q];
                        v += A[6 * r + p] * w;
                    }
                    v *= s2;
                    oc->cov[6 * r + k] = v;
                    oc->cov[6 * k + r] = v;
                }
        } else
            for (int i = 0; i < 36; i++) oc->cov[i] = 0.0;
        oc->sigma_px = sig;
        oc->dof = solved ? (int)dof : 0;
        oc->status = solved ? 0 : 1;
        RigCamRec rc = a.rig[c];
        if (solved) {
            const double *cl = tab + RIG_CAM_DOUBLES * c;
            for (int r = 0; r < 3; r++) {
                rc.E[4 * r] = cl[9 + 3 * r]; rc.E[4 * r + 1] = cl[10 + 3 * r]; rc.E[4 * r + 2] = cl[11 + 3 * r];
                rc.E[4 * r + 3] = cl[18 + r];
            }
        }
        a.rig_out[c] = rc;
    }
    if (tid == 0) {
        RigCalResultRec *r = a.res;
        r->rms_px = status == 0 ? sqrt(st->cost / st->n_corners) : 0.0;
        r->rms_init_px = (status == 0 || status == 3) ? sqrt(st->cost0 / st->n_corners) : 0.0;
        r->sigma_px = sig;
        r->n_frames_used = n; r->n_corners = st->n_corners; r->iterations = st->iterations; r->status = status;
        r->n_solved = ns; r->reserved = 0;
        for (int c = 0; c < 16; c++) {
            r->cam_status[c] = c >= a.n_cams ? 0 : c == 0 ? 1 : ((st->reach >> c) & 1) ? 0 : 2;
            r->cam_frames[c] = c < a.n_cams ? st->cam_frames[c] : 0;
        }
    }
    for (int f = tid; f < a.n_frames; f += CAL_WG) {
        const int *fr = a.fr + RC_FR * f;
        CamPoseRec *o = a.out + f;
        if (fr[0] != 0) continue;  // the seed's record as it is
        if (status == 1 || !fr[4]) { o->status = 5; continue; }
        if (status != 0) { o->status = 4; continue; }
        const double *P = a.pose + ((size_t)cur * a.n_frames + f) * 12, *R = P, *t = P + 9;
        for (int r = 0; r < 3; r++) {
            o->T[4 * r] = R[r]; o->T[4 * r + 1] = R[3 + r]; o->T[4 * r + 2] = R[6 + r];
            o->T[4 * r + 3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
        }
        o->rms_px = sqrt(a.H[((size_t)cur * a.n_frames + f) * a.hs + 27] / (4.0 * fr[2]));
        o->n_tags = fr[2]; o->n_rejected = 0; o->status = 0;
    }
}
