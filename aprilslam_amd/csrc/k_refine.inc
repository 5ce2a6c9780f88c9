// S6 and the hand-over to S7: per-quad edge refinement on the full-resolution image (k_refine: one wavefront per candidate
// quad), then the refined lines, corners and the homography (k_homography: eight lanes per quad).  In k_refine lanes take
// the independent edge samples; designated lanes do the small ordered reductions, so that every float sum has the same
// order as a scalar loop.  The full-resolution gray value is computed on demand from the BGR frame (gray_at), so the
// full-resolution gray image is never materialised in HBM.

// Prologue of the three per-quad kernels: the number of entries of quad_list to walk.  A batch whose work buffers
// overflowed has none (batch_poisoned: the host grows the buffers and runs it again).
__device__ __forceinline__ unsigned int tail_quad_count(const long long *counters, unsigned int max_clusters)
{
    if (batch_poisoned(counters)) return 0;
    const long long nq64 = counters[CNT_NQUADS];
    return nq64 > (long long)max_clusters ? max_clusters : (unsigned int)nq64;
}

// A sample of an edge is probed at the offsets t_j = -(range + 1) + j / 4 along the edge's normal, range = f + 1 for the
// decimation f: steps = 8 (f + 1) + 1 pairs (t_k, t_k+8), so nprobe = 8 (f + 1) + 9 = 25, 33, 41, 49 for f = 1, 2, 3, 4.
#define DEC_PROBE_GROUP 11 /* probes fetched together, so that a group's loads are in flight at once */
#define DEC_MAX_PROBES 44  /* probes a lane parks in LDS: covers decimate <= 3 (41); decimate >= 4 takes refine_walk_steps */
// A probe that lands on a pixel boundary to within rounding error reads the pixel above it
// (pixel-aligned edges put every fourth probe there; tests/golden/README.md).
#define PIX_EPS 9.5367431640625e-07 /* 2^-20 px */

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

// ---- Storage plan of k_refine: the workgroup's LDS, one wavefront.  The kernel holds one RefineStore; the steps reach
// it only through their argument.  Nothing shares memory.  Barriers: L opens a quad (loop top), A follows the corners,
// A' the edge frames, B closes a pass's samples, C closes a pass.
//
//   member   bytes   holds                       written by                      read by                        free after
//   P        64      corners, full resolution    load_corners: lanes 0-3         edge_frames, sample_site (all  L of the next quad
//                                                                                lanes, behind A), hand_over
//   enx/eny  64      unit normal of edge e       edge_frames: lanes 0-3          sample_site (behind A')        L of the next quad
//   soff     20      first sample of edge e in   edge_frames: lane 0             sample_site, edge_sums, the    L of the next quad
//                    the quad's index space;                                     pass loop (behind A')
//                    soff[4] = all samples
//   probe    5632    [probe j][lane]: gray, or   probes_clear / probes_guarded:  weigh_steps: the same lane,    no barrier: a lane
//                    -1 outside the frame        the lane's own column           its own column                 reads only what it wrote
//   bx/by    1024    a pass's refined sample     the sample lanes (walk or       edge_sums: lanes 0-3           C (the next pass or
//   bvalid   256     points and whether the      weigh result), before B         (behind B)                     quad writes them again)
//                    sample found an edge
//   sum      7060    + 4 of padding = 7064, what the build reports
struct RefineStore {
    double P[4][2];
    double enx[4], eny[4];
    double bx[64], by[64];  // one pass of 64 (edge, sample) pairs
    int bvalid[64];
    int soff[5];
    short probe[DEC_MAX_PROBES][64];
};
static_assert(sizeof(RefineStore) == 7064, "k_refine: the plan and the LDS allocation disagree");

// what a lane knows of its sample: the edge, the point on the edge, the edge's normal
struct RefineSite { int edge; double x0, y0, nx, ny; };
// the running sums of an edge's refined points (lane = edge), in sample order
struct RefineSums { double Mx, My, Mxx, Mxy, Myy, Nn; };

// ---- The steps of k_refine, in order.  None ends with a barrier: the kernel body places them.

// Corners of the quad at full resolution.  Lanes 0-3 write P.
__device__ __forceinline__ void refine_load_corners(RefineStore &st, const QuadRec *qp, const Geom &g, int lane)
{
    if (lane < 4) {
        double px = qp->p[lane][0], py = qp->p[lane][1];
        if (g.f > 1) { px = (px - 0.5) * g.f + 0.5; py = (py - 0.5) * g.f + 0.5; }
        st.P[lane][0] = px;
        st.P[lane][1] = py;
    }
}

// Per edge (lanes 0-3): the unit normal, pointing from black to white, and ns = max(16, |edge| / 8) samples; lane 0 writes the
// exclusive prefix of the four counts.  Reads P.
__device__ __forceinline__ void refine_edge_frames(RefineStore &st, int q_reversed, int lane)
{
    if (lane < 4) {
        int edge = lane, a = edge, b = (edge + 1) & 3;
        double nx = st.P[b][1] - st.P[a][1], ny = -st.P[b][0] + st.P[a][0];
        double mag = sqrt(nx * nx + ny * ny);
        nx /= mag; ny /= mag;
        if (q_reversed) { nx = -nx; ny = -ny; }
        int ns = (int)(mag / 8);
        if (ns < 16) ns = 16;
        st.enx[edge] = nx; st.eny[edge] = ny;
        int n0 = __shfl(ns, 0), n1 = __shfl(ns, 1), n2 = __shfl(ns, 2), n3 = __shfl(ns, 3);
        if (lane == 0) { st.soff[0] = 0; st.soff[1] = n0; st.soff[2] = n0 + n1; st.soff[3] = n0 + n1 + n2; st.soff[4] = n0 + n1 + n2 + n3; }
    }
}

// Sample idx of the quad's index space -> its edge, its point on the edge and the edge's normal.  Reads P, enx/eny, soff.
__device__ __forceinline__ RefineSite refine_sample_site(const RefineStore &st, int idx)
{
    const int *soff = st.soff;
    RefineSite s;
    s.edge = idx >= soff[3] ? 3 : (idx >= soff[2] ? 2 : (idx >= soff[1] ? 1 : 0));
    int sidx = idx - soff[s.edge];
    int a = s.edge, b = (s.edge + 1) & 3;
    double pax = st.P[a][0], pay = st.P[a][1], pbx = st.P[b][0], pby = st.P[b][1];
    s.nx = st.enx[s.edge]; s.ny = st.eny[s.edge];
    int nsamples = soff[s.edge + 1] - soff[s.edge];
    double alpha = (1.0 + sidx) / (nsamples + 1);
    s.x0 = alpha * pax + (1 - alpha) * pbx;
    s.y0 = alpha * pay + (1 - alpha) * pby;
    return s;
}

// The probes.  The two probes of step k sit at offsets n + 1 and n - 1 along the normal with n = -range + k / 4, so all
// probes lie on one grid of nprobe = steps + 8 offsets t_j = -(range + 1) + j / 4: they are fetched up front (one latency,
// not one per step) and parked in the lane's column of st.probe ([probe][lane]: conflict-free), in groups of
// DEC_PROBE_GROUP; step k then reads g1 = probe[k + 8], g2 = probe[k].  The offsets are exact in binary (t = tb + u / 4
// too), so the pixel addresses are those of the step-by-step formulation (refine_walk_steps).
//
// The "clear" condition: a sample is clear when its first and its last probe lie in [0, w-2] x [0, h-1].  Probe
// coordinates are monotone in t (every operation of x0 + t * nx + eps and the truncation is), so then all its probes do.
// When that holds for every sample of the wavefront -- any tag away from the frame's border; the kernel asks with
// __all, so the choice is wave-uniform -- refine_probes_clear needs no bounds test, no substitute address, no last-pixel
// fix-up (x + 1 is a pixel of the row: the 4-byte BGR fetch stays inside it) and no "outside" marker: a third of the
// instructions of the loop that is 60 % of this kernel.  Otherwise refine_probes_guarded takes the whole wavefront.
__device__ __forceinline__ bool refine_sample_clear(const RefineSite &s, const Geom &g, double range, int nprobe)
{
    const double t_first = -(range + 1), t_last = -(range + 1) + 0.25 * (nprobe - 1);
    const int xa = (int)(s.x0 + t_first * s.nx + PIX_EPS), xb = (int)(s.x0 + t_last * s.nx + PIX_EPS);
    const int ya = (int)(s.y0 + t_first * s.ny + PIX_EPS), yb = (int)(s.y0 + t_last * s.ny + PIX_EPS);
    return min(xa, xb) >= 0 && max(xa, xb) <= g.w - 2 && min(ya, yb) >= 0 && max(ya, yb) <= g.h - 1;
}

// Probes are a quarter of a pixel apart: three of four land on the pixel of the probe before.  Only a probe on a new
// pixel fetches (a load instruction costs the memory pipeline one access per active lane, and every lane's pixel sits in
// a cache line of its own); the others copy their predecessor.  Writes the lane's column of probe.
template <int CH>
__device__ __forceinline__ void refine_probes_clear(RefineStore &st, const RefineSite &s, const uint8_t *frame, const Geom &g, double range, int nprobe, int lane)
{
    unsigned int at_prev = 0xFFFFFFFFu;
    int gray_prev = 0;
    for (int j0 = 0; j0 < nprobe; j0 += DEC_PROBE_GROUP) {
        const double tb = -(range + 1) + 0.25 * j0;
        unsigned int raw[DEC_PROBE_GROUP], at[DEC_PROBE_GROUP];
#pragma unroll
        for (int u = 0; u < DEC_PROBE_GROUP; u++) {
            const double t = tb + 0.25 * u;
            const int xi = (int)(s.x0 + t * s.nx + PIX_EPS), yi = (int)(s.y0 + t * s.ny + PIX_EPS);
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
                st.probe[j0 + u][lane] = (short)gray_prev;
            }
        }
        at_prev = at[DEC_PROBE_GROUP - 1];
    }
}

// Every probe tested against the frame; one outside is parked as -1 (its fetch goes to pixel (0, 0): unconditional, no
// branch between the fetches).  Writes the lane's column of probe.
template <int CH>
__device__ __forceinline__ void refine_probes_guarded(RefineStore &st, const RefineSite &s, const uint8_t *frame, const Geom &g, double range, int nprobe, int lane)
{
    for (int j0 = 0; j0 < nprobe; j0 += DEC_PROBE_GROUP) {
        unsigned int raw[DEC_PROBE_GROUP], shv[DEC_PROBE_GROUP];
        bool inside[DEC_PROBE_GROUP];
#pragma unroll
        for (int u = 0; u < DEC_PROBE_GROUP; u++) {
            double t = -(range + 1) + 0.25 * (j0 + u);
            int xi = (int)(s.x0 + t * s.nx + PIX_EPS), yi = (int)(s.y0 + t * s.ny + PIX_EPS);
            inside[u] = j0 + u < nprobe && (unsigned int)xi < (unsigned int)g.w && (unsigned int)yi < (unsigned int)g.h;
            raw[u] = pixel_fetch<CH>(frame, g, inside[u] ? xi : 0, inside[u] ? yi : 0, &shv[u]);
        }
#pragma unroll
        for (int u = 0; u < DEC_PROBE_GROUP; u++)
            if (j0 + u < nprobe) st.probe[j0 + u][lane] = inside[u] ? (short)pixel_gray<CH>(raw[u], shv[u]) : (short)-1;
    }
}

// The weighted mean offset of the sample's edge from the parked probes: Mn = sum weight * n, Mcount = sum weight.
// weight = (g2 - g1)^2 is an integer <= 255^2 and n = (k - 4 range) / 4 a multiple of 1/4 below 2^3: every product and
// every partial sum of the scalar loop is exact in double (< 2^27 quarter units), so the sums are carried as integers and
// converted once -- same bits, no f64 work in the loop.  Reads the lane's column of probe.
__device__ __forceinline__ void refine_weigh_steps(const RefineStore &st, int f, int steps, int lane, double *Mn, double *Mcount)
{
    int isum = 0, wsum = 0;
    const int k0 = 4 * (f + 1);
    for (int k = 0; k < steps; k++) {
        const int g1 = st.probe[k + 8][lane], g2 = st.probe[k][lane];
        const int dg = g2 - g1;
        const int wgt = (g1 < 0 || g2 < 0 || g1 < g2) ? 0 : dg * dg;
        isum += wgt * (k - k0);
        wsum += wgt;
    }
    *Mn = 0.25 * (double)isum;
    *Mcount = (double)wsum;
}

// decimate >= 4 (nprobe > DEC_MAX_PROBES): the scalar formulation, two probes per step, nothing parked.
template <int CH>
__device__ __forceinline__ void refine_walk_steps(const RefineSite &s, const uint8_t *frame, const Geom &g, double range, int steps, double *Mn_out, double *Mcount_out)
{
    double Mn = 0, Mcount = 0;
    for (int k = 0; k < steps; k++) {
        double n = -range + 0.25 * k;
        int x1 = (int)(s.x0 + (n + 1) * s.nx + PIX_EPS), y1 = (int)(s.y0 + (n + 1) * s.ny + PIX_EPS);
        if (x1 < 0 || x1 >= g.w || y1 < 0 || y1 >= g.h) continue;
        int x2 = (int)(s.x0 + (n - 1) * s.nx + PIX_EPS), y2 = (int)(s.y0 + (n - 1) * s.ny + PIX_EPS);
        if (x2 < 0 || x2 >= g.w || y2 < 0 || y2 >= g.h) continue;
        int g1 = gray_at<CH>(frame, g, x1, y1), g2 = gray_at<CH>(frame, g, x2, y2);
        if (g1 < g2) continue;
        double weight = (double)((g2 - g1) * (g2 - g1));
        Mn += weight * n;
        Mcount += weight;
    }
    *Mn_out = Mn;
    *Mcount_out = Mcount;
}

// The sample's refined point, the site moved along the normal by the mean offset; none where no step had weight.
// Writes the lane's slot of bx/by/bvalid.
__device__ __forceinline__ void refine_park_sample(RefineStore &st, const RefineSite &s, double Mn, double Mcount, int lane)
{
    if (Mcount == 0) { st.bvalid[lane] = 0; }
    else {
        double n0 = Mn / Mcount;
        st.bx[lane] = s.x0 + n0 * s.nx;
        st.by[lane] = s.y0 + n0 * s.ny;
        st.bvalid[lane] = 1;
    }
}

// Ordered accumulation of the pass [base, base + 64), one lane per edge (lanes 0-3): the lane adds the pass's samples of
// its edge in sample order, so over the passes every sum sees the additions of a scalar loop over the edge.  Reads
// soff, bx/by/bvalid.
__device__ __forceinline__ void refine_edge_sums(const RefineStore &st, int base, int lane, RefineSums &m)
{
    if (lane < 4) {
        const int edge = lane;
        const int lo = (st.soff[edge] > base ? st.soff[edge] : base) - base;
        const int hi = (st.soff[edge + 1] < base + 64 ? st.soff[edge + 1] : base + 64) - base;
        for (int k = lo; k < hi; k++) {
            if (!st.bvalid[k]) continue;
            double bx = st.bx[k], by = st.by[k];
            m.Mx += bx; m.My += by; m.Mxx += bx * bx; m.Mxy += bx * by; m.Myy += by * by; m.Nn++;
        }
    }
}

// Hand-over to k_homography: the corners, and slot 9 = 0.25 (edge sums waiting in edge_mom) or 0.5 (corners final).  Reads P.
__device__ __forceinline__ void refine_hand_over(const RefineStore &st, double *Hout, unsigned int ci, int refine, int lane)
{
    if (lane < 8) Hout[10 * (size_t)ci + lane] = st.P[lane >> 1][lane & 1];
    if (lane == 0) Hout[10 * (size_t)ci + 9] = refine ? 0.25 : 0.5;
}

// S6: edge refinement.  One wavefront per candidate quad; writes the corners and the edge sums for k_homography.
// Split from the decoding so that each half keeps a small register footprint (more wavefronts in flight to hide
// the latency of the scattered pixel probes).
// The (edge, sample) pairs of all four edges form one index space, walked 64 at a time (one pass for a typical tag:
// 4 x 16 samples).  The two `continue`s sit before any barrier of the quad and test fields of the quad's record, the
// same for every lane; the loop-top barrier L keeps the next quad's writes behind this quad's last reads.
template <int CH>
__global__ void __launch_bounds__(64) k_refine(const QuadRec *__restrict__ quads, const long long *__restrict__ counters,
                                               unsigned int max_clusters, const uint8_t *__restrict__ frames, Geom g, int want_polarity /* bit 0: normal, bit 1: reversed */,
                                               int refine, double *__restrict__ Hout /* 10 doubles per cluster: the four corners, 0.25 / 0.5 */,
                                               const unsigned int *__restrict__ quad_list, double *__restrict__ edge_mom /* 4 x 6 per cluster */)
{
    __shared__ RefineStore st;
    const int lane = threadIdx.x;
    PHASE_DECL();
    const unsigned int nq = tail_quad_count(counters, max_clusters);

    for (unsigned int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();  // L
        PHASE_INIT();
        const unsigned int ci = quad_list[qi];
        // fields are read straight from memory: a by-value QuadRec indexed with `lane` would live in scratch memory
        const QuadRec *qp = quads + ci;
        const int q_valid = qp->valid, q_reversed = qp->reversed_border;
        if (lane == 0) Hout[10 * (size_t)ci + 9] = 0.0;
        if (!q_valid) continue;
        if (!((want_polarity >> (q_reversed ? 1 : 0)) & 1)) continue;
        const uint8_t *frame = frames + (size_t)(int)(qp->key >> 48) * g.frame_pitch;
        refine_load_corners(st, qp, g, lane);
        __syncthreads();  // A
        PHASE(16);
        if (refine) {
            refine_edge_frames(st, q_reversed, lane);
            __syncthreads();  // A'
            PHASE(24);
            const double range = g.f + 1;
            const int steps = (int)(2 * range * 4) + 1;
            const int nprobe = steps + 8;
            RefineSums m = {0, 0, 0, 0, 0, 0};
            const int total = st.soff[4];
            for (int base = 0; base < total; base += 64) {
                if (base + lane < total) {
                    const RefineSite s = refine_sample_site(st, base + lane);
                    double Mn, Mcount;
                    if (nprobe <= DEC_MAX_PROBES) {
                        if (__all(refine_sample_clear(s, g, range, nprobe))) refine_probes_clear<CH>(st, s, frame, g, range, nprobe, lane);
                        else refine_probes_guarded<CH>(st, s, frame, g, range, nprobe, lane);
                        PHASE(25);
                        refine_weigh_steps(st, g.f, steps, lane, &Mn, &Mcount);
                    } else {
                        refine_walk_steps<CH>(s, frame, g, range, steps, &Mn, &Mcount);
                    }
                    refine_park_sample(st, s, Mn, Mcount, lane);
                }
                __syncthreads();  // B
                PHASE(26);
                refine_edge_sums(st, base, lane, m);
                __syncthreads();  // C
                PHASE(27);
            }
            // the sums of every edge go to k_homography, which finishes the lines and intersects them (a serial
            // double-precision chain of four independent items: there it runs for eight quads per wavefront)
            if (lane < 4) {
                double *out = edge_mom + ((size_t)ci * 4 + lane) * 6;
                out[0] = m.Mx; out[1] = m.My; out[2] = m.Mxx; out[3] = m.Mxy; out[4] = m.Myy; out[5] = m.Nn;
            }
        }
        PHASE(17);
        refine_hand_over(st, Hout, ci, refine, lane);
        PHASE(22);
    }
    PHASE_FLUSH(16);
}

// S7, first part: the homography of a quad, 8x9 Gaussian elimination with partial pivoting -- EIGHT LANES PER QUAD (lane r
// of a group keeps row r of the system in registers), eight quads per wavefront.  The elimination is a chain of eight
// dependent pivot steps and eight dependent substitutions with a handful of active lanes each: run by a whole wavefront
// per quad (round 2) it was a quarter of k_refine's instructions.  Every matrix element goes through exactly the
// operations of the scalar loop in the same order, so the result is bit-identical to it:
//   pivot of column c = the row at position >= c with the largest |A[.][c]|, the first of them on ties; rows are not
//   moved: a lane carries its row's position `pos` and the "swap" exchanges two positions;
//   f = A[i][c] / A[c][c];  A[i][j] = A[i][j] - f * A[c][j] for j > c;
//   x[c] = (A[c][8] - sum_{i>c} A[c][i] * x[i]) / A[c][c], the sum in ascending i from 0.
// The pivot row and the solved unknowns travel through ds_bpermute (source lane from a ballot); maxima and ties through
// the grp8 primitives of k_wave.inc.  corners_H: 10 doubles per cluster -- in: the four refined corners and 0.5 in
// slot 9 (k_refine); out: H[0..8] and 1.0 (or 0.0 for a singular system).
__global__ void __launch_bounds__(256) k_homography(double *__restrict__ corners_H, const long long *__restrict__ counters, unsigned int max_clusters,
                                                    const unsigned int *__restrict__ quad_list, const double *__restrict__ edge_mom)
{
    const unsigned int nq = tail_quad_count(counters, max_clusters);
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
