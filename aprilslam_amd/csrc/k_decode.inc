// S6-S7: per-quad edge refinement on the full-resolution image (k_refine), the refined lines, corners and the
// homography (k_homography: eight lanes per quad), bit decoding and code-book match (k_decode).  k_refine and k_decode
// run one wavefront per candidate quad: lanes take the independent samples (edge samples, border samples, the 41
// payload bits, the buckets of the code-book index), designated lanes do the small ordered reductions so that every
// float sum has the same order as a scalar loop.
// The full-resolution gray value is computed on demand from the BGR frame (gray_at), so the
// full-resolution gray image is never materialised in HBM.

#define DEC_PROBE_GROUP 11
#define DEC_MAX_PROBES 44  /* decimate <= 3: 33 steps + 8; larger decimations take the generic loop */

__device__ __forceinline__ void half_angle_normal_dev(double a, double b, double *nx, double *ny)
{
    double r = sqrt(a * a + b * b);
    if (r == 0) { *nx = 1; *ny = 0; return; }
    double c2 = a / r;
    if (c2 >= 0) {
        double c = sqrt((1 + c2) / 2);
        *nx = c;
        *ny = b / (2 * r * c);
    } else {
        double s = sqrt((1 - c2) / 2);
        if (b < 0) s = -s;
        *ny = s;
        *nx = b / (2 * r * s);
    }
}

// S7: the homography of a quad, 8x9 Gaussian elimination with partial pivoting -- EIGHT LANES PER QUAD (lane r of a group
// keeps row r of the system in registers), eight quads per wavefront.  The elimination is a chain of eight dependent
// pivot steps and eight dependent substitutions with a handful of active lanes each: run by a whole wavefront per quad
// (round 2) it was a quarter of k_refine's instructions.  Every matrix element goes through exactly the operations of
// the scalar loop in the same order, so the result is bit-identical to it:
//   pivot of column c = the row at position >= c with the largest |A[.][c]|, the first of them on ties; rows are not
//   moved: a lane carries its row's position `pos` and the "swap" exchanges two positions;
//   f = A[i][c] / A[c][c];  A[i][j] = A[i][j] - f * A[c][j] for j > c;
//   x[c] = (A[c][8] - sum_{i>c} A[c][i] * x[i]) / A[c][c], the sum in ascending i from 0.
// The pivot row and the solved unknowns travel through ds_bpermute (source lane from a ballot); maxima and ties through
// DPP (xor 1, xor 2, half-row mirror).  corners_H: 10 doubles per cluster -- in: the four refined corners and 0.5 in
// slot 9 (k_refine); out: H[0..8] and 1.0 (or 0.0 for a singular system).
__device__ __forceinline__ double grp8_max(double v)  // maximum over the 8 lanes of a group, in all of them
{
    v = fmax(v, dpp_mov<QUAD_XOR1>(0.0, v));
    v = fmax(v, dpp_mov<QUAD_XOR2>(0.0, v));
    return fmax(v, dpp_mov<0x141>(0.0, v));  // row_half_mirror: lane i <-> 7 - i, the other quad of the group
}
__device__ __forceinline__ int grp8_min(int v)
{
    v = min(v, dpp_mov<QUAD_XOR1>(0, v));
    v = min(v, dpp_mov<QUAD_XOR2>(0, v));
    return min(v, dpp_mov<0x141>(0, v));
}
// value of the group's lane for which `mine` holds (exactly one per group), in all 8 lanes
__device__ __forceinline__ int grp8_owner(bool mine, int lane)
{
    const unsigned long long m = __ballot(mine);
    return (lane & ~7) + (__ffs((int)((m >> (lane & ~7)) & 0xFFull)) - 1);
}

__global__ void __launch_bounds__(256) k_homography(double *__restrict__ corners_H, const long long *__restrict__ counters, unsigned int max_clusters,
                                                    const unsigned int *__restrict__ quad_list, const double *__restrict__ edge_mom)
{
    if (batch_poisoned(counters)) return;
    const long long nq64 = counters[CNT_NQUADS];
    const unsigned int nq = nq64 > (long long)max_clusters ? max_clusters : (unsigned int)nq64;
    const int lane = threadIdx.x & 63, r = lane & 7;
    for (unsigned int q0 = blockIdx.x * 32u; q0 < nq; q0 += gridDim.x * 32u) {
        const unsigned int qi = q0 + (threadIdx.x >> 3);
        const bool live = qi < nq;
        const unsigned int ci = quad_list[live ? qi : 0];
        double *const rec = corners_H + 10 * (size_t)ci;
        const double state = live ? rec[9] : 0.0;
        const bool todo = state == 0.5 || state == 0.25;
        // S6, last part (state 0.25): lane e < 4 of the group turns the sums of edge e into its line (centroid and the
        // half-angle normal), corner e + 1 is the intersection of the lines e and e + 1 -- kept as it was when the lines
        // are close to parallel.  Lanes 4..7 run along on copies.
        const int e = r & 3;
        double Pex = todo ? rec[2 * e] : 0.0, Pey = todo ? rec[2 * e + 1] : 0.0;  // corner e
        if (__any(state == 0.25)) {
            const double *in = edge_mom + ((size_t)(state == 0.25 ? ci : 0) * 4 + e) * 6;
            const double Mx = in[0], My = in[1], Mxx = in[2], Mxy = in[3], Myy = in[4], Nn = in[5];
            const double Ex = Mx / Nn, Ey = My / Nn;
            const double Cxx = Mxx / Nn - Ex * Ex, Cxy = Mxy / Nn - Ex * Ey, Cyy = Myy / Nn - Ey * Ey;
            double nx, ny;
            half_angle_normal_dev(Cyy - Cxx, -2 * Cxy, &nx, &ny);
            // lines e (own) and e + 1 (next lane of the quad) -> corner e + 1
            const double n0 = dpp_mov<QUAD_ROT1>(0.0, Ex), n1 = dpp_mov<QUAD_ROT1>(0.0, Ey), n2 = dpp_mov<QUAD_ROT1>(0.0, nx), n3 = dpp_mov<QUAD_ROT1>(0.0, ny);
            const double A00 = ny, A01 = -n3;
            const double A10 = -nx, A11 = n2;
            const double B0 = -Ex + n0;
            const double B1 = -Ey + n1;
            const double det = A00 * A11 - A10 * A01;
            const bool moved = fabs(det) > 0.001;
            const double W00 = A11 / det, W01 = -A01 / det;
            const double L0 = W00 * B0 + W01 * B1;
            const double cx = Ex + L0 * A00, cy = Ey + L0 * A10;
            // corner e comes from the lane of edge e - 1
            const double fx = dpp_mov<QUAD_ROT3>(0.0, cx), fy = dpp_mov<QUAD_ROT3>(0.0, cy);
            const bool fm = dpp_mov<QUAD_ROT3>(0, moved ? 1 : 0) != 0;
            if (state == 0.25 && fm) { Pex = fx; Pey = fy; }
        }
        // row r: corner i = r / 2; even rows the x equation, odd rows the y equation
        const int i = r >> 1;
        const double x = (i == 1 || i == 2) ? 1.0 : -1.0, y = (i >= 2) ? 1.0 : -1.0;
        const double u = __shfl(Pex, (lane & ~7) + i), v = __shfl(Pey, (lane & ~7) + i);
        double a[9];
        if ((r & 1) == 0) { a[0] = x; a[1] = y; a[2] = 1; a[3] = 0; a[4] = 0; a[5] = 0; a[6] = -x * u; a[7] = -y * u; a[8] = u; }
        else { a[0] = 0; a[1] = 0; a[2] = 0; a[3] = x; a[4] = y; a[5] = 1; a[6] = -x * v; a[7] = -y * v; a[8] = v; }
        int pos = r;
        bool ok = true;
#pragma unroll
        for (int col = 0; col < 8; col++) {
            const double val = pos >= col ? fabs(a[col]) : -1.0;
            const double mx = grp8_max(val);
            if (mx < 1e-10) ok = false;  // singular: the group carries on (no lane may leave the exchanges), its result is dropped
            const int pivpos = grp8_min(val == mx ? pos : 99);
            const bool is_piv = pos == pivpos;
            if (is_piv) pos = col;
            else if (pos == col) pos = pivpos;
            const int src = grp8_owner(is_piv, lane);
            double piv[9];
#pragma unroll
            for (int j = col; j < 9; j++) piv[j] = __shfl(a[j], src);
            if (pos > col) {
                const double f = a[col] / piv[col];
                a[col] = 0.0;
#pragma unroll
                for (int j = col + 1; j < 9; j++) a[j] = a[j] - f * piv[j];
            }
        }
        double xs[8], mine = 0;
#pragma unroll
        for (int col = 7; col >= 0; col--) {
            double sum = 0;
#pragma unroll
            for (int k = col + 1; k < 8; k++) sum += a[k] * xs[k];
            const double xc = (a[8] - sum) / a[col];
            xs[col] = __shfl(xc, grp8_owner(pos == col, lane));
            if (r == col) mine = xs[col];
        }
        const bool all_ok = (__ballot(ok) >> (lane & ~7) & 0xFFull) == 0xFFull;  // every lane of the group saw the same maxima
        if (todo) {
            rec[r] = mine;
            if (r == 0) { rec[8] = 1.0; rec[9] = all_ok ? 1.0 : 0.0; }
        }
    }
}

__device__ __forceinline__ void hproject_dev(const double *H, double x, double y, double *ox, double *oy)
{
    double xx = H[0] * x + H[1] * y + H[2];
    double yy = H[3] * x + H[4] * y + H[5];
    double zz = H[6] * x + H[7] * y + H[8];
    *ox = xx / zz;
    *oy = yy / zz;
}

struct GrayModel { double A[9], B[3], C[3]; };

__device__ __forceinline__ void gm_add_dev(GrayModel &gm, double x, double y, double gray)
{
    gm.A[0] += x * x; gm.A[1] += x * y; gm.A[2] += x; gm.A[4] += y * y; gm.A[5] += y; gm.A[8] += 1;
    gm.B[0] += x * gray; gm.B[1] += y * gray; gm.B[2] += gray;
}

__device__ __forceinline__ void gm_solve_dev(GrayModel &gm)
{
    const double *A = gm.A, *B = gm.B;
    double L[9], M[9], t[3];
    L[0] = sqrt(A[0]); L[3] = A[1] / L[0]; L[6] = A[2] / L[0];
    L[4] = sqrt(A[4] - L[3] * L[3]); L[7] = (A[5] - L[3] * L[6]) / L[4];
    L[8] = sqrt(A[8] - L[6] * L[6] - L[7] * L[7]);
    M[0] = 1 / L[0]; M[3] = -L[3] * M[0] / L[4]; M[4] = 1 / L[4];
    M[6] = (-L[6] * M[0] - L[7] * M[3]) / L[8]; M[7] = -L[7] * M[4] / L[8]; M[8] = 1 / L[8];
    t[0] = M[0] * B[0]; t[1] = M[3] * B[0] + M[4] * B[1]; t[2] = M[6] * B[0] + M[7] * B[1] + M[8] * B[2];
    gm.C[0] = M[0] * t[0] + M[3] * t[1] + M[6] * t[2];
    gm.C[1] = M[4] * t[1] + M[7] * t[2];
    gm.C[2] = M[8] * t[2];
}

__device__ __forceinline__ double gm_interp_dev(const GrayModel &gm, double x, double y) { return gm.C[0] * x + gm.C[1] * y + gm.C[2]; }

template <int CH>
__device__ __forceinline__ double value_for_pixel_dev(const uint8_t *frame, const Geom &g, double px, double py)
{
    int x1 = (int)floor(px - 0.5), x2 = (int)ceil(px - 0.5);
    double x = px - 0.5 - x1;
    int y1 = (int)floor(py - 0.5), y2 = (int)ceil(py - 0.5);
    double y = py - 0.5 - y1;
    if (x1 < 0 || x2 >= g.w || y1 < 0 || y2 >= g.h) return -1;
    return gray_at<CH>(frame, g, x1, y1) * (1 - x) * (1 - y) + gray_at<CH>(frame, g, x2, y1) * x * (1 - y) +
           gray_at<CH>(frame, g, x1, y2) * (1 - x) * y + gray_at<CH>(frame, g, x2, y2) * x * y;
}

__device__ __forceinline__ unsigned long long rotate90_dev(unsigned long long w, int nbits)
{
    int p = nbits;
    unsigned long long l = 0;
    if (nbits % 4 == 1) { p = nbits - 1; l = 1; }
    w = ((w >> l) << (p / 4 + l)) | (w >> (3 * p / 4 + l) << l) | (w & l);
    w &= ((1ull << nbits) - 1ull);
    return w;
}

// A probe that lands on a pixel boundary to within rounding error reads the pixel above it
// (pixel-aligned edges put every fourth probe there; tests/golden/README.md).
#define PIX_EPS 9.5367431640625e-07 /* 2^-20 px */

// S6: edge refinement.  One wavefront per candidate quad; writes the refined corners for k_homography.
// Split from the decoding so that each half keeps a small register footprint (more wavefronts in flight to hide
// the latency of the scattered pixel probes).
template <int CH>
__global__ void __launch_bounds__(64) k_refine(const QuadRec *__restrict__ quads, const long long *__restrict__ counters,
                                               unsigned int max_clusters, const uint8_t *__restrict__ frames, Geom g, int fam_reversed,
                                               int refine, double *__restrict__ Hout /* 10 doubles per cluster: the four corners, 0.25 / 0.5 */,
                                               const unsigned int *__restrict__ quad_list, double *__restrict__ edge_mom /* 4 x 6 per cluster */)
{
    __shared__ double s_bx[64], s_by[64];  // one pass of 64 (edge, sample) pairs
    __shared__ int s_bvalid[64];
    __shared__ double s_P[4][2];
    __shared__ int s_soff[5];
    __shared__ short s_probe[DEC_MAX_PROBES][64];
    __shared__ double s_enx[4], s_eny[4];
    int lane = threadIdx.x;
    PHASE_DECL();
    if (batch_poisoned(counters)) return;
    long long nq64 = counters[CNT_NQUADS];
    unsigned int nq = nq64 > (long long)max_clusters ? max_clusters : (unsigned int)nq64;

    for (unsigned int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();
        PHASE_INIT();
        const unsigned int ci = quad_list[qi];
        // fields are read straight from memory: a by-value QuadRec indexed with `lane` would live in scratch memory
        const QuadRec *qp = quads + ci;
        const int q_valid = qp->valid, q_reversed = qp->reversed_border;
        if (lane == 0) Hout[10 * (size_t)ci + 9] = 0.0;
        if (!q_valid) continue;
        if (fam_reversed != q_reversed) continue;
        int fr = (int)(qp->key >> 48);
        const uint8_t *frame = frames + (size_t)fr * g.frame_pitch;
        if (lane < 4) {
            double px = qp->p[lane][0], py = qp->p[lane][1];
            if (g.f > 1) { px = (px - 0.5) * g.f + 0.5; py = (py - 0.5) * g.f + 0.5; }
            s_P[lane][0] = px;
            s_P[lane][1] = py;
        }
        __syncthreads();

        PHASE(16);
        // ---- S6 refine edges: all (edge, sample) pairs are spread over the lanes at once
        if (refine) {
            if (lane < 4) {
                int edge = lane, a = edge, b = (edge + 1) & 3;
                double nx = s_P[b][1] - s_P[a][1], ny = -s_P[b][0] + s_P[a][0];
                double mag = sqrt(nx * nx + ny * ny);
                nx /= mag; ny /= mag;
                if (q_reversed) { nx = -nx; ny = -ny; }
                int ns = (int)(mag / 8);
                if (ns < 16) ns = 16;
                s_enx[edge] = nx; s_eny[edge] = ny;
                // exclusive prefix over the four edges
                int n0 = __shfl(ns, 0), n1 = __shfl(ns, 1), n2 = __shfl(ns, 2), n3 = __shfl(ns, 3);
                if (lane == 0) { s_soff[0] = 0; s_soff[1] = n0; s_soff[2] = n0 + n1; s_soff[3] = n0 + n1 + n2; s_soff[4] = n0 + n1 + n2 + n3; }
            }
            __syncthreads();
            PHASE(24);
            const int *soff = s_soff;
            const double *enx = s_enx, *eny = s_eny;
            const double range = g.f + 1;
            const int steps = (int)(2 * range * 4) + 1;
            const int nprobe = steps + 8;
            // The (edge, sample) pairs of all four edges form one index space, walked 64 at a time (one pass for a
            // typical tag: 4 x 16 samples).  After each pass the four accumulator lanes (lane = edge) add the pass's
            // samples of their edge in sample order, so every sum sees the additions of a scalar loop over the edge.
            double Mx = 0, My = 0, Mxx = 0, Mxy = 0, Myy = 0, Nn = 0;
            const int total = soff[4];
            for (int base = 0; base < total; base += 64) {
            {
                const int idx = base + lane;
                if (idx < total) {
                int edge = idx >= soff[3] ? 3 : (idx >= soff[2] ? 2 : (idx >= soff[1] ? 1 : 0));
                int sidx = idx - soff[edge];
                int a = edge, b = (edge + 1) & 3;
                double pax = s_P[a][0], pay = s_P[a][1], pbx = s_P[b][0], pby = s_P[b][1];
                double nx = enx[edge], ny = eny[edge];
                int nsamples = soff[edge + 1] - soff[edge];
                double alpha = (1.0 + sidx) / (nsamples + 1);
                double x0 = alpha * pax + (1 - alpha) * pbx;
                double y0 = alpha * pay + (1 - alpha) * pby;
                double Mn = 0, Mcount = 0;
                // The two probes of step k sit at offsets n+1 and n-1 along the normal with
                // n = -range + k/4, so all probes lie on one grid of steps+8 offsets
                // t_j = -(range+1) + j/4: fetch them up front (one latency, not one per step);
                // step k then reads g1 = v[k+8], g2 = v[k].  Offsets are exact in binary, so the
                // pixel addresses are those of the step-by-step formulation.
                if (nprobe <= DEC_MAX_PROBES) {
                    // probes parked in LDS ([probe][lane]: conflict-free), so neither loop needs unrolling
                    // and the kernel keeps a small register footprint
                    // fetched in groups of DEC_PROBE_GROUP so that a group's loads are in flight together
                    //
                    // Probe coordinates are monotone in t (every operation of x0 + t * nx + eps and the truncation is),
                    // so when the two end probes of a sample lie in [0, w-2] x [0, h-1] all its probes do: if that holds
                    // for every sample of the wavefront -- any tag away from the frame's border -- the probes need no
                    // bounds test, no substitute address, no last-pixel fix-up and no "outside" marker: a third of
                    // the instructions of the loop that is 60 % of this kernel.  t = tb + u / 4 is exact either way.
                    const double t_first = -(range + 1), t_last = -(range + 1) + 0.25 * (nprobe - 1);
                    const int xa = (int)(x0 + t_first * nx + PIX_EPS), xb = (int)(x0 + t_last * nx + PIX_EPS);
                    const int ya = (int)(y0 + t_first * ny + PIX_EPS), yb = (int)(y0 + t_last * ny + PIX_EPS);
                    const bool clear = min(xa, xb) >= 0 && max(xa, xb) <= g.w - 2 && min(ya, yb) >= 0 && max(ya, yb) <= g.h - 1;
                    if (__all(clear)) {
                        // Probes are a quarter of a pixel apart: three of four land on the pixel of the probe before.  Only a
                        // probe on a new pixel fetches (a load instruction costs the memory pipeline one access per active
                        // lane, and every lane's pixel sits in a cache line of its own); the others copy their predecessor.
                        unsigned int at_prev = 0xFFFFFFFFu;
                        int gray_prev = 0;
                        for (int j0 = 0; j0 < nprobe; j0 += DEC_PROBE_GROUP) {
                            const double tb = -(range + 1) + 0.25 * j0;
                            unsigned int raw[DEC_PROBE_GROUP], at[DEC_PROBE_GROUP];
#pragma unroll
                            for (int u = 0; u < DEC_PROBE_GROUP; u++) {
                                const double t = tb + 0.25 * u;
                                const int xi = (int)(x0 + t * nx + PIX_EPS), yi = (int)(y0 + t * ny + PIX_EPS);
                                at[u] = j0 + u < nprobe ? (unsigned int)yi * (unsigned int)g.stride + (unsigned int)(CH * xi) : 0xFFFFFFFEu;
                            }
#pragma unroll
                            for (int u = 0; u < DEC_PROBE_GROUP; u++) {
                                raw[u] = 0;
                                if (j0 + u < nprobe && at[u] != (u ? at[u - 1] : at_prev)) {
                                    if (CH == 1) raw[u] = frame[at[u]];
                                    else __builtin_memcpy(&raw[u], frame + at[u], 4);
                                }
                            }
#pragma unroll
                            for (int u = 0; u < DEC_PROBE_GROUP; u++) {
                                if (j0 + u < nprobe) {
                                    const bool fresh = at[u] != (u ? at[u - 1] : at_prev);
                                    gray_prev = fresh ? (CH == 1 ? (int)raw[u] : bgr_gray(raw[u])) : gray_prev;
                                    s_probe[j0 + u][lane] = (short)gray_prev;
                                }
                            }
                            at_prev = at[DEC_PROBE_GROUP - 1];
                        }
                    } else
                    for (int j0 = 0; j0 < nprobe; j0 += DEC_PROBE_GROUP) {
                        unsigned int raw[DEC_PROBE_GROUP], shv[DEC_PROBE_GROUP];
                        bool inside[DEC_PROBE_GROUP];
#pragma unroll
                        for (int u = 0; u < DEC_PROBE_GROUP; u++) {
                            double t = -(range + 1) + 0.25 * (j0 + u);
                            int xi = (int)(x0 + t * nx + PIX_EPS), yi = (int)(y0 + t * ny + PIX_EPS);
                            inside[u] = j0 + u < nprobe && (unsigned int)xi < (unsigned int)g.w && (unsigned int)yi < (unsigned int)g.h;
                            raw[u] = pixel_fetch<CH>(frame, g, inside[u] ? xi : 0, inside[u] ? yi : 0, &shv[u]);  // unconditional: no branch between the fetches
                        }
#pragma unroll
                        for (int u = 0; u < DEC_PROBE_GROUP; u++)
                            if (j0 + u < nprobe) s_probe[j0 + u][lane] = inside[u] ? (short)pixel_gray<CH>(raw[u], shv[u]) : (short)-1;
                    }
                    PHASE(25);
                    // weight = (g2 - g1)^2 is an integer <= 255^2 and n = (k - 4 range) / 4 a multiple of 1/4 below 2^3: every
                    // product and every partial sum of the scalar loop is exact in double (< 2^27 quarter units), so the
                    // sums can be carried as integers and converted once -- same bits, no f64 work in the loop
                    int isum = 0, wsum = 0;
                    const int k0 = 4 * (g.f + 1);
                    for (int k = 0; k < steps; k++) {
                        const int g1 = s_probe[k + 8][lane], g2 = s_probe[k][lane];
                        const int dg = g2 - g1;
                        const int wgt = (g1 < 0 || g2 < 0 || g1 < g2) ? 0 : dg * dg;
                        isum += wgt * (k - k0);
                        wsum += wgt;
                    }
                    Mn = 0.25 * (double)isum;
                    Mcount = (double)wsum;
                } else {  // decimate >= 3: step-by-step probes
                    for (int k = 0; k < steps; k++) {
                        double n = -range + 0.25 * k;
                        int x1 = (int)(x0 + (n + 1) * nx + PIX_EPS), y1 = (int)(y0 + (n + 1) * ny + PIX_EPS);
                        if (x1 < 0 || x1 >= g.w || y1 < 0 || y1 >= g.h) continue;
                        int x2 = (int)(x0 + (n - 1) * nx + PIX_EPS), y2 = (int)(y0 + (n - 1) * ny + PIX_EPS);
                        if (x2 < 0 || x2 >= g.w || y2 < 0 || y2 >= g.h) continue;
                        int g1 = gray_at<CH>(frame, g, x1, y1), g2 = gray_at<CH>(frame, g, x2, y2);
                        if (g1 < g2) continue;
                        double weight = (double)((g2 - g1) * (g2 - g1));
                        Mn += weight * n;
                        Mcount += weight;
                    }
                }
                if (Mcount == 0) { s_bvalid[lane] = 0; }
                else {
                    double n0 = Mn / Mcount;
                    s_bx[lane] = x0 + n0 * nx;
                    s_by[lane] = y0 + n0 * ny;
                    s_bvalid[lane] = 1;
                }
                }
            }
            __syncthreads();
            PHASE(26);
            // ordered accumulation of this pass, one lane per edge
            if (lane < 4) {
                const int edge = lane;
                const int lo = (soff[edge] > base ? soff[edge] : base) - base;
                const int hi = (soff[edge + 1] < base + 64 ? soff[edge + 1] : base + 64) - base;
                for (int k = lo; k < hi; k++) {
                    if (!s_bvalid[k]) continue;
                    double bx = s_bx[k], by = s_by[k];
                    Mx += bx; My += by; Mxx += bx * bx; Mxy += bx * by; Myy += by * by; Nn++;
                }
            }
            __syncthreads();
            PHASE(27);
            }  // passes
            // the four sums of every edge go to k_homography, which finishes the lines and intersects them (a serial
            // double-precision chain of four independent items: there it runs for eight quads per wavefront)
            if (lane < 4) {
                double *out = edge_mom + ((size_t)ci * 4 + lane) * 6;
                out[0] = Mx; out[1] = My; out[2] = Mxx; out[3] = Mxy; out[4] = Myy; out[5] = Nn;
            }
        }

        PHASE(17);
        // ---- hand over to k_homography: the corners, and slot 9 = 0.25 (edge sums waiting in edge_mom) or 0.5 (corners final)
        if (lane < 8) Hout[10 * (size_t)ci + lane] = s_P[lane >> 1][lane & 1];
        if (lane == 0) Hout[10 * (size_t)ci + 9] = refine ? 0.25 : 0.5;
        PHASE(22);
    }
    PHASE_FLUSH(16);
}

// 5 waves per SIMD (96 VGPRs, 24 bytes of scratch) beats the 4 the allocator picks on its own; 6 spills too much
template <int CH>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) k_decode(const QuadRec *__restrict__ quads, const double *__restrict__ Hin,
                                               const long long *__restrict__ counters, unsigned int max_clusters,
                                               const uint8_t *__restrict__ frames, Geom g, FamilyDev fam, int maxhamming, DetRec *dets,
                                               unsigned int max_dets, long long *wcounters, const unsigned int *__restrict__ quad_list)
{
    __shared__ double s_H[9];
    __shared__ double s_smp[40][4];  // tagx, tagy, v, 1
    __shared__ double s_values[16 * 16], s_list[2 * 64];  // payload cells; the white and the black values in bit order
    __shared__ double s_smpxy[40][2], s_bitxy[64][2];
    __shared__ GrayModel s_white, s_black;
    __shared__ int s_ok;
    int lane = threadIdx.x;
    PHASE_DECL();
    if (batch_poisoned(counters)) return;
    long long nq64 = counters[CNT_NQUADS];
    unsigned int nq = nq64 > (long long)max_clusters ? max_clusters : (unsigned int)nq64;

    // Tag-frame coordinates of the 40 border samples and of the payload bits depend on the family only: computed once per
    // workgroup (the pattern switch, two integer and four double divisions per lane), read from LDS for every quad.
    {
        const int wb = fam.width_at_border;
        if (lane < 8 * wb && lane < 40) {
            int pi = lane / wb, i = lane % wb;
            double p0, p1, p2, p3;
            switch (pi) {
            case 0: p0 = -0.5; p1 = 0.5; p2 = 0; p3 = 1; break;
            case 1: p0 = 0.5; p1 = 0.5; p2 = 0; p3 = 1; break;
            case 2: p0 = wb + 0.5; p1 = .5; p2 = 0; p3 = 1; break;
            case 3: p0 = wb - 0.5; p1 = .5; p2 = 0; p3 = 1; break;
            case 4: p0 = 0.5; p1 = -0.5; p2 = 1; p3 = 0; break;
            case 5: p0 = 0.5; p1 = 0.5; p2 = 1; p3 = 0; break;
            case 6: p0 = 0.5; p1 = wb + 0.5; p2 = 1; p3 = 0; break;
            default: p0 = 0.5; p1 = wb - 0.5; p2 = 1; p3 = 0; break;
            }
            double tagx01 = (p0 + i * p2) / wb, tagy01 = (p1 + i * p3) / wb;
            s_smpxy[lane][0] = 2 * (tagx01 - 0.5);
            s_smpxy[lane][1] = 2 * (tagy01 - 0.5);
        }
        if (lane < fam.nbits) {
            int bitx = fam.bit_x[lane], bity = fam.bit_y[lane];
            double tagx01 = (bitx + 0.5) / wb, tagy01 = (bity + 0.5) / wb;
            s_bitxy[lane][0] = 2 * (tagx01 - 0.5);
            s_bitxy[lane][1] = 2 * (tagy01 - 0.5);
        }
    }
    for (unsigned int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();
        PHASE_INIT();
        const unsigned int ci = quad_list[qi];
        if (Hin[10 * (size_t)ci + 9] == 0.0) continue;  // no quad, wrong polarity, or singular homography
        unsigned long long qkey = quads[ci].key;
        int fr = (int)(qkey >> 48);
        const uint8_t *frame = frames + (size_t)fr * g.frame_pitch;
        if (lane < 9) s_H[lane] = Hin[10 * (size_t)ci + lane];
        __syncthreads();
        int wb = fam.width_at_border, tw = fam.total_width;

        PHASE(18);
        // border samples: 8 patterns x wb samples
        int nsmp = 8 * wb;
        if (lane < nsmp && lane < 40) {
            const double tagx = s_smpxy[lane][0], tagy = s_smpxy[lane][1];
            double px, py;
            hproject_dev(s_H, tagx, tagy, &px, &py);
            int ix = (int)px, iy = (int)py;
            // a sample outside the frame is left out of the sums upstream: here its row is all zeros, so that each of its
            // terms is +0.0 and leaves a sum that started at +0.0 exactly as it is (no flag to read in the loop below)
            const bool inside = !(ix < 0 || iy < 0 || ix >= g.w || iy >= g.h);
            const double gv = (double)gray_at<CH>(frame, g, inside ? ix : 0, inside ? iy : 0);
            s_smp[lane][0] = inside ? tagx : 0.0; s_smp[lane][1] = inside ? tagy : 0.0; s_smp[lane][2] = inside ? gv : 0.0; s_smp[lane][3] = inside ? 1.0 : 0.0;
        }
        __syncthreads();
        {
            // Gray models of the white and the black border.  Upstream adds the samples one by one into 9 running sums
            // per model; here lane a (0..8: white, 9..17: black) owns one sum and walks the samples in the same order,
            // so every sum sees the same additions -- 40 steps of a wavefront instead of 40 x 9 of a single lane.
            // The sum's term is u*v with u, v picked from the sample's (x, y, gray, 1) row (x*1 and 1*1 are exact).
            const int a = lane % 9, m = lane / 9;
            const int ku = a <= 2 ? 0 : (a <= 4 ? 1 : (a == 5 ? 3 : (a == 6 ? 0 : (a == 7 ? 1 : 2))));
            const int kv = a == 0 ? 0 : (a == 1 ? 1 : (a == 3 ? 1 : (a == 6 || a == 7 ? 2 : 3)));
            double acc = 0;
            if (lane < 18) {
                // patterns alternate white, black: a model's lanes visit only their own patterns (half the samples), in order
                const int ns = nsmp < 40 ? nsmp : 40;
                for (int p0 = m * wb; p0 < ns; p0 += 2 * wb) {
                    const int pe = p0 + wb < ns ? p0 + wb : ns;
                    for (int smp = p0; smp < pe; smp++) {
                        const double u = s_smp[smp][ku], v = s_smp[smp][kv];
                        acc += u * v;
                    }
                }
            }
            // both models are solved at once: lane 0 solves white, lane 1 black (every lane runs the same code on its copy)
            GrayModel gm;
            const int base = (lane & 1) * 9;
            gm.A[0] = __shfl(acc, base + 0); gm.A[1] = __shfl(acc, base + 1); gm.A[2] = __shfl(acc, base + 2);
            gm.A[3] = 0; gm.A[4] = __shfl(acc, base + 3); gm.A[5] = __shfl(acc, base + 4);
            gm.A[6] = 0; gm.A[7] = 0; gm.A[8] = __shfl(acc, base + 5);
            gm.B[0] = __shfl(acc, base + 6); gm.B[1] = __shfl(acc, base + 7); gm.B[2] = __shfl(acc, base + 8);
            gm.C[0] = 0; gm.C[1] = 0; gm.C[2] = 0;
            gm_solve_dev(gm);
            if (lane == 0) s_white = gm;
            if (lane == 1) s_black = gm;
            const double at0 = gm_interp_dev(gm, 0, 0);
            const double w0 = __shfl(at0, 0), b0 = __shfl(at0, 1);
            if (lane == 0) {
                bool flip = (w0 - b0 < 0);
                s_ok = (flip == (fam.reversed_border != 0)) ? 1 : 0;
            }
        }
        for (int i = lane; i < tw * tw; i += 64) s_values[i] = 0;
        __syncthreads();
        if (!s_ok) continue;

        PHASE(19);
        // payload bits
        int min_coord = (wb - tw) / 2;
        int bit_cell = 0, cell_x = 0, cell_y = 0;  // this lane's payload bit sits in s_values[bit_cell], cell (cell_x, cell_y) of the tag
        if (lane < fam.nbits) {
            int bitx = fam.bit_x[lane], bity = fam.bit_y[lane];
            cell_x = bitx - min_coord; cell_y = bity - min_coord;
            bit_cell = tw * cell_y + cell_x;
            const double tagx = s_bitxy[lane][0], tagy = s_bitxy[lane][1];
            double px, py;
            hproject_dev(s_H, tagx, tagy, &px, &py);
            double v = value_for_pixel_dev<CH>(frame, g, px, py);
            if (v != -1) {
                double thresh = (gm_interp_dev(s_black, tagx, tagy) + gm_interp_dev(s_white, tagx, tagy)) / 2.0;
                s_values[bit_cell] = v - thresh;
            }
        }
        __syncthreads();
        // Sharpening (upstream: the whole tw x tw grid through a 3x3 Laplacian, then value + 0.25 * Laplacian): only the payload
        // cells are read afterwards, so each bit's lane sharpens its own cell -- the same five terms in the same order.
        // No second grid, no pass over the 81 cells (two rounds with an integer division each), two barriers fewer.
        double sharp_v = 0.0;
        if (lane < fam.nbits) {
            double sv = 0;
            if (cell_y - 1 >= 0) sv += s_values[bit_cell - tw] * -1.0;
            if (cell_x - 1 >= 0) sv += s_values[bit_cell - 1] * -1.0;
            sv += s_values[bit_cell] * 4.0;
            if (cell_x + 1 <= tw - 1) sv += s_values[bit_cell + 1] * -1.0;
            if (cell_y + 1 <= tw - 1) sv += s_values[bit_cell + tw] * -1.0;
            sharp_v = s_values[bit_cell] + 0.25 * sv;
        }

        PHASE(20);
        // code word + decision margin (ordered float sums: every lane repeats them, 41 steps)
        // Upstream walks the bits in order and adds each value to the white or the black score (a float that takes a
        // double: rounded after every addition).  The two scores are independent chains, so lane 0 adds the white values
        // in bit order and lane 1 the negated black ones, from two compacted lists -- ~20 steps of one add instead of 41
        // steps of compare, two conversions, add and select by every lane.  The code word is the ballot of "white".
        float black_score, white_score, black_count, white_count;
        unsigned long long rcode;
        {
            const bool isbit = lane < fam.nbits;
            const double v = isbit ? sharp_v : 0.0;
            const bool isw = isbit && v > 0;
            const unsigned long long wm = __ballot(isw), bm = __ballot(isbit && !isw);
            rcode = __brevll(wm) >> (64 - fam.nbits);  // bit 0 of the family is the most significant bit of the code
            const unsigned long long below = (1ull << lane) - 1ull;
            if (isbit) s_list[isw ? __popcll(wm & below) : 64 + __popcll(bm & below)] = isw ? v : -v;
            __syncthreads();
            float score = 0;
            if (lane < 2) {
                const int cnt = lane == 0 ? __popcll(wm) : __popcll(bm);
                const double *list = s_list + 64 * lane;
                for (int k = 0; k < cnt; k++) score = (float)((double)score + list[k]);
            }
            white_score = __shfl(score, 0);
            black_score = __shfl(score, 1);
            white_count = (float)(1 + __popcll(wm));
            black_count = (float)(1 + __popcll(bm));
        }
        // code book: first rotation whose best match is within maxhamming; ties -> lowest id
        int id = -1, hamming = 255, rotation = 0;
        if (fam.idx_nch > 0) {
            // lane (rotation, chunk) looks its bucket up; the best candidate of the lowest rotation wins -- what the search of
            // the whole book below returns: its first rotation with a code within maxhamming, lowest distance, lowest id
            unsigned int best = 0xFFFFFFFFu;
            const int ridx = lane >> 2, c = lane & 3;
            unsigned long long rr = rcode;  // the word turned ridx times
#pragma unroll
            for (int k = 1; k < 4; k++) {
                const unsigned long long t = rotate90_dev(rr, fam.nbits);
                rr = ridx >= k ? t : rr;
            }
            if (lane < 16 && c < fam.idx_nch) {
                const int lo = c == 0 ? fam.idx_lo[0] : (c == 1 ? fam.idx_lo[1] : (c == 2 ? fam.idx_lo[2] : fam.idx_lo[3]));
                const int w = c == 0 ? fam.idx_w[0] : (c == 1 ? fam.idx_w[1] : (c == 2 ? fam.idx_w[2] : fam.idx_w[3]));
                const unsigned int b = idx_bucket((rr >> lo) & ((1ull << w) - 1ull), w);
                const unsigned short *st = fam.idx_start + (size_t)c * (IDX_BUCKETS + 1) + b;
                const unsigned long long *ent = fam.idx_entries + (size_t)c * fam.ncodes;
                const unsigned int k1 = st[1];
                for (unsigned int k = st[0]; k < k1; k++) {
                    const unsigned long long en = ent[k];
                    const unsigned int dd = (unsigned int)__popcll(rr ^ (en & 0xFFFFFFFFFFFFull));
                    const unsigned int packed = ((unsigned int)ridx << 24) | (dd << 16) | (unsigned int)(en >> 48);
                    if (dd <= (unsigned int)maxhamming && packed < best) best = packed;
                }
            }
            best = wave_scan<true>(best, 0xFFFFFFFFu, [](unsigned int a, unsigned int b2) { return a < b2 ? a : b2; });
            if (best != 0xFFFFFFFFu) { id = (int)(best & 0xFFFFu); hamming = (int)((best >> 16) & 0xFFu); rotation = (int)(best >> 24); }
        } else {
            // no index (a family wider than 48 bits): every rotation against the whole book
            for (int ridx = 0; ridx < 4; ridx++) {
                unsigned int best = 0xFFFFFFFFu;
                for (int i = lane; i < fam.ncodes; i += 64) {
                    unsigned int dd = (unsigned int)__popcll(rcode ^ fam.codes[i]);
                    unsigned int packed = (dd << 16) | (unsigned int)i;
                    best = packed < best ? packed : best;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    unsigned int o = (unsigned int)__shfl_xor((int)best, off);
                    best = o < best ? o : best;
                }
                if ((best >> 16) <= (unsigned int)maxhamming) { id = (int)(best & 0xFFFFu); hamming = (int)(best >> 16); rotation = ridx; break; }
                rcode = rotate90_dev(rcode, fam.nbits);
            }
        }
        PHASE(21);
        float margin = fminf(white_score / white_count, black_score / black_count);
        if (!(margin >= 0) || hamming >= 255) continue;

        if (lane == 0) {
            unsigned int di = (unsigned int)atomicAdd((unsigned long long *)&wcounters[CNT_NDETS], 1ull);
            if (di >= max_dets) { atomicAdd((unsigned long long *)&wcounters[CNT_OVERFLOW_DETS], 1ull); }
            else {
                const double C[4] = {1, 0, -1, 0}, Sn[4] = {0, 1, 0, -1};
                double c = C[rotation], s = Sn[rotation], Hr[9];
                for (int r = 0; r < 3; r++) {
                    Hr[3 * r + 0] = s_H[3 * r + 0] * c + s_H[3 * r + 1] * s;
                    Hr[3 * r + 1] = s_H[3 * r + 0] * -s + s_H[3 * r + 1] * c;
                    Hr[3 * r + 2] = s_H[3 * r + 2];
                }
                DetRec *d = &dets[di];
                d->id = id; d->hamming = hamming; d->margin = margin; d->frame = fr; d->key = qkey;
                d->pose_ok = 0; d->pad = 0;
                hproject_dev(Hr, 0, 0, &d->center[0], &d->center[1]);
                for (int i = 0; i < 4; i++) {
                    int tcx = (i == 1 || i == 2) ? 1 : -1, tcy = (i < 2) ? 1 : -1;
                    hproject_dev(Hr, tcx, tcy, &d->corners[i][0], &d->corners[i][1]);
                }
            }
        }
        PHASE(23);
    }
    PHASE_FLUSH(16);
}
