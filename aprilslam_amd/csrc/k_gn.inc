// Pose-graph Levenberg-Marquardt back-end (row G of SURVEY.md section 8a) -- NOT in the reference
// (slam_graph.py:72-76 is a stub); build-defined; the tests hold a NumPy restatement of the same step.
//
// Unknowns: camera poses W_f (camera<-world) and tag poses G_j (world<-tag), 12 doubles each (R row-major, t).
// Observation m = (camera f, tag j, 4 pixel corners); residual = projection of W_f G_j X_k minus the corner, 8 per
// observation (asl_gn_solve: pinhole; the map solver, k_map.inc: the k_pnp.inc lens model).  Left-multiplicative updates
// (omega, v): R <- exp(omega) R, t <- exp(omega) t + v.
//
// One LM step on the device (gn_host.inc enqueues the whole loop, gn_lm_run, for both solvers):
//   gn_obs_block     one wavefront per observation (in k_gn_linearize / k_map_linearize, with their camera model): the
//                    8 x 12 Jacobian [J_cam | J_tag] and the residual in registers, the 12 x 12 normal block J^T J with
//                    J^T r as a 13th column from TWO v_mfma_f64_16x16x4_f64 issues (K = 8 = 2 x 4: used, not filled)
//   k_gn_reduce_cam  per-camera sums of the observation blocks in observation order (deterministic, no float
//                    atomics), LM damping, 6x6 camera inverses
//   k_gn_schur       reduced tag system S = H_ll - sum_f W_fj^T H_cc^-1 W_fj', rhs likewise
//   k_gn_chol_*      blocked dense Cholesky of S (diagonal block, panel, MFMA trailing update per block column); the rhs
//                    rides along as row n, so the forward substitution comes out of it
//   k_gn_trisolve    the back substitution;  k_gn_update  camera steps, trial poses
//   k_gn_cost, k_gn_decide (gn_accept: cost down, lambda *= 0.1; else lambda *= 10), k_gn_commit (an accepted trial)
typedef double gn_v4d __attribute__((ext_vector_type(4)));

#define GN_DSTRIDE 156  /* 12 x 13 doubles per observation */
// LM state in device memory, so that a whole solve is enqueued without a host round trip per iteration
enum { GN_LM_COST = 0, GN_LM_TRIAL, GN_LM_LAMBDA, GN_LM_ACCEPTED, GN_LM_FLAG, GN_LM_COST0, GN_LM__N = 8 };

__device__ __forceinline__ void gn_exp_rot(const double *w, double *R)
{
    double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (th < 1e-300) { R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1; return; }
    double x = w[0] / th, y = w[1] / th, z = w[2] / th, c = cos(th), s = sin(th), c1 = 1 - c;
    // I + s K + (1-c) K^2
    R[0] = 1 + c1 * (-(y * y + z * z)); R[1] = -s * z + c1 * x * y;       R[2] = s * y + c1 * x * z;
    R[3] = s * z + c1 * x * y;          R[4] = 1 + c1 * (-(x * x + z * z)); R[5] = -s * x + c1 * y * z;
    R[6] = -s * y + c1 * x * z;         R[7] = s * x + c1 * y * z;        R[8] = 1 + c1 * (-(x * x + y * y));
}

// One observation's 12 x 13 block [J^T J | J^T r] at Dm, by one wavefront, for the poses Wf (camera<-world) and Gj
// (world<-tag); returns the observation's cost in lane 0.  Residual rows k = kk, kk + 4 (corner k >> 1, component k & 1)
// are the K slices of the two MFMA issues: A[i][k] = J[k][i], B[k][j] = [J | r][k][j].  row(k, p, jp, add), the camera
// model at the camera-frame corner p, returns residual k and writes d u / d p (row k & 1) to jp, the row's cost to add.
template <class Row>
__device__ __forceinline__ double gn_obs_block(const double *Wf, const double *Gj, double half, int lane, Row row, double *Dm)
{
    const int n = lane & 15, kk = lane >> 4;
    gn_v4d acc = {0, 0, 0, 0};
    double rsq = 0;
#pragma unroll
    for (int step = 0; step < 2; step++) {
        const int k = kk + 4 * step;
        const int corner = k >> 1;
        const double ox = (corner == 1 || corner == 2) ? half : -half, oy = (corner >= 2) ? half : -half;
        double q[3], p[3];
#pragma unroll
        for (int r = 0; r < 3; r++) q[r] = Gj[3 * r] * ox + Gj[3 * r + 1] * oy + Gj[9 + r];
#pragma unroll
        for (int r = 0; r < 3; r++) p[r] = Wf[3 * r] * q[0] + Wf[3 * r + 1] * q[1] + Wf[3 * r + 2] * q[2] + Wf[9 + r];
        double jp[3], add;
        const double res = row(k, p, jp, add);
        // camera block: dp/d(omega,v) = [-[p]x | I]  ->  jp * that
        double Jrow[12];
        Jrow[0] = p[1] * jp[2] - p[2] * jp[1];   // jp (-[p]x) = (p x jp)^T
        Jrow[1] = p[2] * jp[0] - p[0] * jp[2];
        Jrow[2] = p[0] * jp[1] - p[1] * jp[0];
        Jrow[3] = jp[0]; Jrow[4] = jp[1]; Jrow[5] = jp[2];
        // tag block: dp/d(omega,v) = R_W [-[q]x | I]; let a = R_W^T jp, then row = [q x a | a]
        double a[3];
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = Wf[c] * jp[0] + Wf[3 + c] * jp[1] + Wf[6 + c] * jp[2];
        Jrow[6] = q[1] * a[2] - q[2] * a[1];
        Jrow[7] = q[2] * a[0] - q[0] * a[2];
        Jrow[8] = q[0] * a[1] - q[1] * a[0];
        Jrow[9] = a[0]; Jrow[10] = a[1]; Jrow[11] = a[2];
        double sel = 0;
#pragma unroll
        for (int c = 0; c < 12; c++) sel = (n == c) ? Jrow[c] : sel;
        double av = n < 12 ? sel : 0.0;
        double bv = n < 12 ? sel : (n == 12 ? res : 0.0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        if (n == 0) rsq += add;  // one lane per residual row
    }
    // Dm[row][col]: lane holds rows (lane>>4) + 4i, column lane&15
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int r = kk + 4 * i;
        if (r < 12 && n < 13) Dm[r * 13 + n] = acc[i];
    }
    // cost of this observation: lanes 0,16,32,48 hold two rows each
    double c = rsq;
    c += __shfl_xor(c, 16);
    c += __shfl_xor(c, 32);
    return c;
}

// one wavefront per observation (gn_obs_block, pinhole camera); blockDim = 256 (4 observations per workgroup)
__global__ void __launch_bounds__(256) k_gn_linearize(const double *__restrict__ W, const double *__restrict__ G, const int *__restrict__ obs_cam,
                                                      const int *__restrict__ obs_tag, const double *__restrict__ obs_corners, int n_obs,
                                                      CamDev cam, double *__restrict__ D, double *__restrict__ cost_obs)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n_obs) return;
    const double *corners = obs_corners + 8 * (size_t)m;
    auto row = [=](int k, const double *p, double *jp, double &add) {
        const int comp = k & 1;
        double iz = 1.0 / p[2];
        double u = comp == 0 ? cam.fx * p[0] * iz + cam.cx : cam.fy * p[1] * iz + cam.cy;
        double res = u - corners[k];
        jp[0] = comp == 0 ? cam.fx * iz : 0.0;
        jp[1] = comp == 0 ? 0.0 : cam.fy * iz;
        jp[2] = comp == 0 ? -cam.fx * p[0] * iz * iz : -cam.fy * p[1] * iz * iz;
        add = res * res;
        return res;
    };
    const double c = gn_obs_block(W + 12 * (size_t)obs_cam[m], G + 12 * (size_t)obs_tag[m], cam.half, lane, row, D + (size_t)m * GN_DSTRIDE);
    if (lane == 0) cost_obs[m] = c;
}

// deterministic sum of cost_obs by one workgroup
__global__ void __launch_bounds__(256) k_gn_cost(const double *__restrict__ cost_obs, int n_obs, double *__restrict__ out)
{
    __shared__ double s[256];
    double acc = 0;
    for (int i = threadIdx.x; i < n_obs; i += 256) acc += cost_obs[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// the accept rule: a trial that lowers the cost is taken (lambda /= 10, counted), otherwise the current poses stay
// (lambda *= 10); FLAG and the return value say which
__device__ __forceinline__ bool gn_accept(double *lm)
{
    const bool take = lm[GN_LM_TRIAL] < lm[GN_LM_COST];
    if (take) {
        lm[GN_LM_COST] = lm[GN_LM_TRIAL];
        lm[GN_LM_LAMBDA] = fmax(lm[GN_LM_LAMBDA] * 0.1, 1e-12);
        lm[GN_LM_ACCEPTED] += 1.0;
    } else
        lm[GN_LM_LAMBDA] *= 10.0;
    lm[GN_LM_FLAG] = take ? 1.0 : 0.0;
    return take;
}

__global__ void k_gn_decide(double *lm) { gn_accept(lm); }

// an accepted trial becomes the current state: poses and the linearisation that was computed for them
__global__ void __launch_bounds__(256) k_gn_commit(const double *__restrict__ lm, const double *__restrict__ Wt, const double *__restrict__ Gt,
                                                   const double *__restrict__ Dt, double *__restrict__ Wc, double *__restrict__ Gc, double *__restrict__ Dc,
                                                   size_t nw, size_t ng, size_t nd)
{
    if (lm[GN_LM_FLAG] == 0.0) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw + ng + nd; i += (size_t)gridDim.x * blockDim.x) {
        if (i < nw) Wc[i] = Wt[i];
        else if (i < nw + ng) Gc[i - nw] = Gt[i - nw];
        else Dc[i - nw - ng] = Dt[i - nw - ng];
    }
}

__device__ __forceinline__ bool gn_inv6(const double *A, double *Ainv)
{
    // SPD inverse by Cholesky: A = L L^T, Ainv = L^-T L^-1
    double L[36], Li[36];
#pragma unroll
    for (int i = 0; i < 36; i++) { L[i] = 0; Li[i] = 0; }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = A[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k];
            if (i == j) { if (!(s > 0)) return false; L[6 * i + i] = sqrt(s); }
            else L[6 * i + j] = s / L[6 * j + j];
        }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        Li[6 * i + i] = 1.0 / L[6 * i + i];
#pragma unroll
        for (int j = 0; j < i; j++) {
            double s = 0;
#pragma unroll
            for (int k = j; k < i; k++) s -= L[6 * i + k] * Li[6 * k + j];
            Li[6 * i + j] = s / L[6 * i + i];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += Li[6 * k + i] * Li[6 * k + j];
            Ainv[6 * i + j] = s;
        }
    return true;
}

// one thread per camera: H_cc, g_c from its observation list (in order), damping, inverse, T_fj = Hinv W_fj
// one workgroup per camera: thread t < 36 owns entry (t / 6, t % 6) of H_cc, threads 36..41 own g; each walks the camera's
// observations in observation order (deterministic sums); thread 0 damps and inverts; then all threads fill H_cc^-1 W_fj
__global__ void __launch_bounds__(64) k_gn_reduce_cam(const double *__restrict__ D, const int *__restrict__ cam_ptr, const int *__restrict__ cam_obs,
                                                      int n_cams, const double *__restrict__ lm, double *__restrict__ Hinv, double *__restrict__ gc,
                                                      double *__restrict__ Tfj)
{
    __shared__ double sH[36], sHi[36];
    __shared__ int s_ok;
    const int f = blockIdx.x, t = threadIdx.x;
    if (f >= n_cams) return;
    const double lambda = lm[GN_LM_LAMBDA];
    const int b = cam_ptr[f], e = cam_ptr[f + 1];
    if (t < 42) {
        const int off = t < 36 ? (t / 6) * 13 + (t % 6) : (t - 36) * 13 + 12;
        double acc = 0;
        for (int o = b; o < e; o++) acc += D[(size_t)cam_obs[o] * GN_DSTRIDE + off];
        if (t < 36) sH[t] = acc;
        else gc[6 * (size_t)f + (t - 36)] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double H[36], Hi[36];
#pragma unroll
        for (int i = 0; i < 36; i++) H[i] = sH[i];
#pragma unroll
        for (int i = 0; i < 6; i++) H[6 * i + i] += lambda * (H[6 * i + i] > 1e-12 ? H[6 * i + i] : 1e-12);
        bool ok = e > b && gn_inv6(H, Hi);
#pragma unroll
        for (int i = 0; i < 36; i++) sHi[i] = ok ? Hi[i] : 0.0;
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (t < 36) Hinv[36 * (size_t)f + t] = sHi[t];
    for (int idx = t; idx < (e - b) * 36; idx += 64) {
        const int o = b + idx / 36, ij = idx % 36, i = ij / 6, j = ij % 6;
        const int m = cam_obs[o];
        const double *Dm = D + (size_t)m * GN_DSTRIDE;
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += sHi[6 * i + k] * Dm[k * 13 + 6 + j];
        Tfj[36 * (size_t)m + ij] = s;
    }
}

// one workgroup per (tag j, tag j2) block of the reduced system; thread (a,b) of the 6x6 block (+6 threads for the rhs when j == j2)
__global__ void __launch_bounds__(64) k_gn_schur(const double *__restrict__ D, const double *__restrict__ Tfj, const double *__restrict__ Hinv,
                                                 const double *__restrict__ gc, const int *__restrict__ tag_ptr, const int *__restrict__ tag_obs,
                                                 const int *__restrict__ obs_cam, const int *__restrict__ obs_of, int n_cams, int n_tags,
                                                 int fixed_tag, const double *__restrict__ lm, double *__restrict__ S, double *__restrict__ rhs)
{
    int j = blockIdx.x, j2 = blockIdx.y, t = threadIdx.x;
    const double lambda = lm[GN_LM_LAMBDA];
    int n = 6 * n_tags;
    int b = tag_ptr[j], e = tag_ptr[j + 1];
    bool frozen_row = (j == fixed_tag) || (e == b), frozen_col = (j2 == fixed_tag) || (tag_ptr[j2 + 1] == tag_ptr[j2]);
    if (t < 36) {
        int a = t / 6, c = t % 6;
        double s = 0;
        if (frozen_row || frozen_col) s = (j == j2 && a == c) ? 1.0 : 0.0;  // gauge / unobserved: identity rows
        else {
            if (j == j2) {
                for (int o = b; o < e; o++) s += D[(size_t)tag_obs[o] * GN_DSTRIDE + (6 + a) * 13 + 6 + c];
                if (a == c) s += lambda * (s > 1e-12 ? s : 1e-12);
            }
            // - sum over cameras that saw both tags of W_fj^T (Hinv_f W_fj2)
            for (int o = b; o < e; o++) {
                int m = tag_obs[o], f = obs_cam[m];
                int m2 = obs_of[(size_t)f * n_tags + j2];
                if (m2 < 0) continue;
                const double *Wm = D + (size_t)m * GN_DSTRIDE, *T2 = Tfj + 36 * (size_t)m2;
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) acc += Wm[k * 13 + 6 + a] * T2[6 * k + c];
                s -= acc;
            }
        }
        S[(size_t)(6 * j + a) * n + 6 * j2 + c] = s;
    } else if (t < 42 && j == j2) {
        int a = t - 36;
        double s = 0;
        if (!frozen_row) {
            for (int o = b; o < e; o++) s -= D[(size_t)tag_obs[o] * GN_DSTRIDE + (6 + a) * 13 + 12];
            for (int o = b; o < e; o++) {
                int m = tag_obs[o], f = obs_cam[m];
                const double *Wm = D + (size_t)m * GN_DSTRIDE, *Hi = Hinv + 36 * (size_t)f, *g = gc + 6 * (size_t)f;
                double acc = 0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double y = 0;  // (Hinv g)_k
#pragma unroll
                    for (int l = 0; l < 6; l++) y += Hi[6 * k + l] * g[l];
                    acc += Wm[k * 13 + 6 + a] * y;
                }
                s += acc;
            }
        }
        rhs[6 * j + a] = s;
    }
}

// Dense Cholesky S = L L^T in place (lower triangle), right-looking and blocked by GN_NB columns so that the O(n^3)
// part -- the trailing update -- runs on the whole chip: per block column one small launch factors the diagonal
// block, one solves the panel below it, one updates the trailing matrix tile by tile.  (A 200-tag map has n = 1200;
// a single-workgroup factorisation took 300 ms per LM step there.)  The upper triangle is never read afterwards.
#define GN_NB 48
#define GN_LDP (GN_NB + 1) /* odd LDS row pitch: conflict-free column walks */

// One wavefront factors the diagonal block: lane r holds row r in registers (48 doubles), column k travels through LDS
// (every lane writes its entry, then all lanes read the same addresses: broadcasts, no conflicts, no barrier inside a
// wave) and both loops are fully unrolled so every register index is a constant.  The trailing update uses the
// unscaled column and 1/d (a[c] -= (a_rk / d) * a_ck), which keeps the pivot's square root off the critical path.
// L is collected row-major in LDS on the way; with it lane j then solves L x = e_j for column j of L_kk^-1 (again
// broadcast reads): with the inverse the back substitution of a block is a matrix-vector product instead of 48
// dependent steps.  Rows / columns beyond nb (the last, partial block) are padded with the identity.
// The empty asm statements pin each value where it is computed: without them the compiler sinks the whole update chain
// towards its (conditional) stores, keeps every LDS read alive until then and spills ~7 KB per lane.
#define GN_DIAG_LD 50  /* row stride of L in LDS, doubles: even (16-byte aligned pairs) and not a multiple of 32 banks */

__global__ void __launch_bounds__(64) k_gn_chol_diag(double *__restrict__ S, int n, int k0, int nb, int *__restrict__ fail_flag, double *__restrict__ Linv)
{
    __shared__ __attribute__((aligned(16))) double col[64];
    __shared__ __attribute__((aligned(16))) double Ls[GN_NB * GN_DIAG_LD];
    __shared__ double ild[GN_NB];
    const int r = threadIdx.x;
    const int rr = r < GN_NB ? r : GN_NB - 1;  // lanes 48..63 shadow row 47 and never store
    double a[GN_NB];
#pragma unroll
    for (int c = 0; c < GN_NB; c++) a[c] = (rr < nb && c <= rr) ? S[(size_t)(k0 + rr) * n + k0 + c] : ((rr == c) ? 1.0 : 0.0);
    bool bad = false;
#pragma unroll
    for (int k = 0; k < GN_NB; k++) {
        col[r] = a[k];
        __builtin_amdgcn_wave_barrier();
        double d = col[k];
        if (!(d > 0)) { bad = true; d = 1.0; }
        double il = __builtin_amdgcn_rsq(d);           // ~2^-26 relative; two Newton steps reach double precision
        il = il * (1.5 - 0.5 * d * il * il);
        il = il * (1.5 - 0.5 * d * il * il);
        const double t = a[k] * (il * il);              // a_rk / d
        const double lrk = a[k] * il;                   // L[r][k]; rows above the diagonal hold zeros there
        if (r < GN_NB) Ls[r * GN_DIAG_LD + k] = r >= k ? lrk : 0.0;
        if (r == 0) ild[k] = il;
        a[k] = lrk;
        asm("" : "+v"(a[k]));
#pragma unroll
        for (int c = k + 1; c < GN_NB; c++) { a[c] = __builtin_fma(-t, col[c], a[c]); asm("" : "+v"(a[c])); }  // A[r][c] with c > r is never read
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);  // keep the steps apart: hoisted LDS reads of later steps only cost registers
    }
    if (bad && r == 0) *fail_flag = 1;
#pragma unroll
    for (int i = 0; i < GN_NB; i++)
        if (r < nb && i <= r) S[(size_t)(k0 + r) * n + k0 + i] = a[i];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // lane j: column j of L^-1 by forward substitution; x[i] = 0 for i < j falls out of the recurrence
    double x[GN_NB];
#pragma unroll
    for (int i = 0; i < GN_NB; i++) {
        double s = i == r ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) s = __builtin_fma(-Ls[i * GN_DIAG_LD + k], x[k], s);
        x[i] = s * ild[i];
        asm("" : "+v"(x[i]));
        __builtin_amdgcn_sched_barrier(0);
    }
    double *Lb = Linv + (size_t)(k0 / GN_NB) * GN_NB * GN_NB;
#pragma unroll
    for (int i = 0; i < GN_NB; i++) {
        if (r < GN_NB) Lb[i * GN_NB + r] = x[i];
    }
}

// rows below the diagonal block: X L_kk^T = A.  16 lanes share a row (lane j of the group owns columns j, j+16, j+32):
// at step c the owner of column c finishes x_c, broadcasts it, and every lane retires it from its later columns.
__global__ void __launch_bounds__(256) k_gn_chol_panel(double *__restrict__ S, int n, int nrows, int k0, int nb)
{
    __shared__ double Lk[GN_NB][GN_LDP], inv[GN_NB];
    const int t = threadIdx.x, j = t & 15;
    const int row = k0 + nb + blockIdx.x * 16 + (t >> 4);
    for (int i = t; i < nb * nb; i += 256) { int r = i / nb, c = i - r * nb; Lk[r][c] = S[(size_t)(k0 + r) * n + k0 + c]; }
    __syncthreads();
    if (t < nb) inv[t] = 1.0 / Lk[t][t];
    __syncthreads();
    double x[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        int c = j + 16 * b;
        x[b] = (row < nrows && c < nb) ? S[(size_t)row * n + k0 + c] : 0.0;
    }
    for (int c = 0; c < nb; c++) {
        // owner of column c: lane c & 15, slot c >> 4
        const int slot = c >> 4;
        double mine = slot == 0 ? x[0] : (slot == 1 ? x[1] : x[2]);
        double xc = __shfl(mine * inv[c], (t & 48) | (c & 15));
        if (j == (c & 15)) { if (slot == 0) x[0] = xc; else if (slot == 1) x[1] = xc; else x[2] = xc; }
#pragma unroll
        for (int b = 0; b < 3; b++) {
            int dcol = j + 16 * b;
            if (dcol > c && dcol < nb) x[b] -= xc * Lk[dcol][c];
        }
    }
#pragma unroll
    for (int b = 0; b < 3; b++) {
        int c = j + 16 * b;
        if (row < nrows && c < nb) S[(size_t)row * n + k0 + c] = x[b];
    }
}

// trailing update, one GN_NB x GN_NB tile of the lower triangle per workgroup: A_ij -= L_i L_j^T (panel rows i, j) -- the
// O(n^3) part of the factorisation, on the matrix pipe: the tile is 3 x 3 blocks of 16 x 16, a block is nb / 4
// v_mfma_f64_16x16x4_f64 issues (A[m][k] = L_i[m][k], B[k][n] = L_j[n][k]), the nine blocks are dealt to the four wavefronts.
__global__ void __launch_bounds__(256) k_gn_chol_update(double *__restrict__ S, int n, int nrows, int k0, int nb)
{
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double Li[GN_NB][GN_LDP], Lj[GN_NB][GN_LDP];
    const int t = threadIdx.x;
    const int i0 = k0 + nb + blockIdx.x * GN_NB, j0 = k0 + nb + blockIdx.y * GN_NB;
    for (int i = t; i < GN_NB * GN_NB; i += 256) {
        int r = i / GN_NB, c = i - r * GN_NB;
        Li[r][c] = (c < nb && i0 + r < nrows) ? S[(size_t)(i0 + r) * n + k0 + c] : 0.0;  // columns beyond nb are zero: the K loop runs to GN_NB
        Lj[r][c] = (c < nb && j0 + r < n) ? S[(size_t)(j0 + r) * n + k0 + c] : 0.0;
    }
    __syncthreads();
    const int lane = t & 63, wid = t >> 6, m = lane & 15, kk = lane >> 4;
    for (int blk = wid; blk < 9; blk += 4) {
        const int bi = blk / 3, bj = blk - 3 * bi;
        gn_v4d acc = {0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < GN_NB / 4; ks++)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[16 * bi + m][4 * ks + kk], Lj[16 * bj + m][4 * ks + kk], acc, 0, 0, 0);
        // the lane holds rows kk + 4 i of column m of the block
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = i0 + 16 * bi + kk + 4 * i, c = j0 + 16 * bj + m;
            if (r < nrows && c < n && c <= r) S[(size_t)r * n + c] -= acc[i];
        }
    }
}

// L^T x = y, blocked like the factorisation; one workgroup, x lives in LDS (n doubles, dynamic).  The forward substitution
// L y = b needs no pass of its own: b rides along as row n of the matrix through the factorisation (its panel solves and
// trailing updates are exactly the forward substitution), so y is found there.  A block's own unknowns are
// x_b = L_bb^-T r_b with the inverse k_gn_chol_diag left behind (one matrix-vector product, 48 lanes, the inverse staged
// in LDS by everybody); then all threads
// retire x_b from the rows above with contiguous reads of L.  Those reads do not depend on x: every thread issues its 48
// loads of the block's column panel BEFORE the matrix-vector product and consumes them after, so the memory latency of
// the panel and the dependent product overlap and a block costs one latency, not 48/8 of them.
#define GN_TRI_THREADS 512
#define GN_TRI_LPT ((GN_NB * GN_NB + GN_TRI_THREADS - 1) / GN_TRI_THREADS)  /* entries of L_bb^-1 a thread stages */
__global__ void __launch_bounds__(GN_TRI_THREADS) k_gn_trisolve(const double *__restrict__ S, const double *__restrict__ Linv, double *__restrict__ x, int n)
{
    extern __shared__ double xs[];
    __shared__ double xb[GN_NB], Li[GN_NB * GN_NB];
    const int tid = threadIdx.x, nt = GN_TRI_THREADS;
    for (int i = tid; i < n; i += nt) xs[i] = S[(size_t)n * n + i];
    __syncthreads();
    const int nblk = (n + GN_NB - 1) / GN_NB;
    for (int bi = nblk - 1; bi >= 0; bi--) {
        const int k0 = bi * GN_NB, nb = min(GN_NB, n - k0);
        const bool act = tid < k0;
        const double *Lb = Linv + (size_t)bi * GN_NB * GN_NB;
        double lr[GN_TRI_LPT];
#pragma unroll
        for (int q = 0; q < GN_TRI_LPT; q++) lr[q] = tid + q * nt < GN_NB * GN_NB ? Lb[tid + q * nt] : 0.0;
        double pv[GN_NB];
#pragma unroll
        for (int c = 0; c < GN_NB; c++) pv[c] = act ? S[(size_t)min(k0 + c, n - 1) * n + tid] : 0.0;  // rows past nb meet xb = 0
#pragma unroll
        for (int q = 0; q < GN_TRI_LPT; q++)
            if (tid + q * nt < GN_NB * GN_NB) Li[tid + q * nt] = lr[q];
        __syncthreads();
        if (tid < GN_NB) {
            double s = 0;
#pragma unroll 8
            for (int r = 0; r < GN_NB; r++) s += Li[r * GN_NB + tid] * (r < nb ? xs[k0 + r] : 0.0);  // (L^-T r)_c = sum_r L^-1[r][c] r_r
            xb[tid] = tid < nb ? s : 0.0;
        }
        __syncthreads();
        if (tid < nb) xs[k0 + tid] = xb[tid];
        if (act) {
            double s = 0;
#pragma unroll
            for (int c = 0; c < GN_NB; c++) s += pv[c] * xb[c];
            xs[tid] -= s;
        }
        for (int i = tid + nt; i < k0; i += nt) {
            double s = 0;
#pragma unroll 16
            for (int c = 0; c < GN_NB; c++) s += S[(size_t)min(k0 + c, n - 1) * n + i] * xb[c];
            xs[i] -= s;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += nt) x[i] = xs[i];
}

// camera steps and all trial poses; one thread per camera / per tag
__global__ void __launch_bounds__(64) k_gn_update(const double *__restrict__ D, const double *__restrict__ Hinv, const double *__restrict__ gc,
                                                  const int *__restrict__ cam_ptr, const int *__restrict__ cam_obs, const int *__restrict__ obs_tag,
                                                  const double *__restrict__ dG, int n_cams, int n_tags, const double *__restrict__ W,
                                                  const double *__restrict__ G, double *__restrict__ Wn, double *__restrict__ Gn)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    double d[6];
    const double *src;
    double *dst;
    if (i < n_cams) {
        double rhs[6];
#pragma unroll
        for (int a = 0; a < 6; a++) rhs[a] = -gc[6 * (size_t)i + a];
        for (int o = cam_ptr[i]; o < cam_ptr[i + 1]; o++) {
            int m = cam_obs[o];
            const double *Wm = D + (size_t)m * GN_DSTRIDE, *dg = dG + 6 * (size_t)obs_tag[m];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double s = 0;
#pragma unroll
                for (int c = 0; c < 6; c++) s += Wm[a * 13 + 6 + c] * dg[c];
                rhs[a] -= s;
            }
        }
        const double *Hi = Hinv + 36 * (size_t)i;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double s = 0;
#pragma unroll
            for (int c = 0; c < 6; c++) s += Hi[6 * a + c] * rhs[c];
            d[a] = s;
        }
        src = W + 12 * (size_t)i;
        dst = Wn + 12 * (size_t)i;
    } else if (i < n_cams + n_tags) {
        int j = i - n_cams;
#pragma unroll
        for (int a = 0; a < 6; a++) d[a] = dG[6 * (size_t)j + a];
        src = G + 12 * (size_t)j;
        dst = Gn + 12 * (size_t)j;
    } else
        return;
    double R[9];
    gn_exp_rot(d, R);
    // R' = exp(w) R ; t' = exp(w) t + v
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) dst[3 * r + c] = R[3 * r] * src[c] + R[3 * r + 1] * src[3 + c] + R[3 * r + 2] * src[6 + c];
        dst[9 + r] = R[3 * r] * src[9] + R[3 * r + 1] * src[10] + R[3 * r + 2] * src[11] + d[3 + r];
    }
}
