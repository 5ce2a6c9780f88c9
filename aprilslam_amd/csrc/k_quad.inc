// S5: fit a quad to every surviving cluster.
//
// Clusters are small (tens to a few hundred boundary points for a 720p frame) and there are
// ~10^2 of them per frame, so the unit of parallelism is the cluster and the working set lives
// in LDS.  Clusters are filed by size class (k_cluster_filter; CLASSn_CAP of asl_common.h) and launch_fit_class
// (aprilslam.hip) gives every class its instantiation k_fit_quads<NT, PPT>, PPT = cap / NT points per thread:
//   class 0: <= 128 points   <64, 2>    one wavefront per cluster,    8 KB of dynamic LDS
//   class 1: <= 256 points   <128, 2>   two wavefronts per cluster,  16 KB
//   class 2: <= 512 points   <256, 2>   four wavefronts per cluster, 32 KB
//   class 3: <= 1024 points  <256, 4>   four wavefronts per cluster, 64 KB
//   class 4: larger          <256, 0>   four wavefronts per cluster, arrays in the cluster's global slab
// (QUAD_LDS_BYTES(cap): 64 bytes per point and 96 of padding.)  Where the arrays of a cluster lie, and which of them
// share memory, is FitStore's plan below -- the one place that says so.
// Steps (identical arithmetic in every class), one function each, called in this order by k_fit_quads:
//   0. bounding box + integer gradient sums -> box centre, border polarity (early rejects)
//   1. 64-bit sort keys (angle about the centre | y | x), bitonic sort
//   2. drop duplicate points (ordered compaction by ballot/popcount prefix sums)
//   3. gradient weight per point, then the six running line-fit moments.  The moments are a
//      strictly ordered float64 prefix sum: lanes 0..5 each carry one moment sequentially, so
//      the rounding is identical to a scalar loop (bit-exact against the oracle)
//   4. windowed line-fit error per point, 7-tap low-pass, local maxima, keep the 10 strongest
//   5. all C(n,4) corner choices in parallel (n <= 10 maxima), lexicographically-first minimum total error
//   6. the moments of the winner's four sides; their line fits, intersections, area / angle / winding checks are
//      k_quad_finish's (four lanes per cluster, sixteen clusters per wavefront)
// All float math is IEEE without contraction so it can be compared bit for bit with the oracle.

// Corner search over the (at most ten) maxima m_0 < m_1 < ...: a quad is a 4-subset a < b < c < d with sides (a,b), (b,c), (c,d) and
// the side (d,a) that wraps around the outline.
// All 4-subsets of {0..9} ordered by (d, c, b, a), so that the subsets of {0..n-1} are the first C(n,4) entries, packed
// a | b<<4 | c<<8 | d<<12 | rank<<16 with rank = the subset's place in lexicographic order (upstream's loop order: among
// equal errors the earliest combination wins).
__device__ const unsigned int kCombo4of10[210] = {
    0x003210u, 0x014210u, 0x074310u, 0x1c4320u, 0x544321u, 0x025210u, 0x085310u, 0x1d5320u, 0x555321u, 0x0d5410u,
    0x225420u, 0x5a5421u, 0x315430u, 0x695431u, 0x8c5432u, 0x036210u, 0x096310u, 0x1e6320u, 0x566321u, 0x0e6410u,
    0x236420u, 0x5b6421u, 0x326430u, 0x6a6431u, 0x8d6432u, 0x126510u, 0x276520u, 0x5f6521u, 0x366530u, 0x6e6531u,
    0x916532u, 0x406540u, 0x786541u, 0x9b6542u, 0xaf6543u, 0x047210u, 0x0a7310u, 0x1f7320u, 0x577321u, 0x0f7410u,
    0x247420u, 0x5c7421u, 0x337430u, 0x6b7431u, 0x8e7432u, 0x137510u, 0x287520u, 0x607521u, 0x377530u, 0x6f7531u,
    0x927532u, 0x417540u, 0x797541u, 0x9c7542u, 0xb07543u, 0x167610u, 0x2b7620u, 0x637621u, 0x3a7630u, 0x727631u,
    0x957632u, 0x447640u, 0x7c7641u, 0x9f7642u, 0xb37643u, 0x4a7650u, 0x827651u, 0xa57652u, 0xb97653u, 0xc37654u,
    0x058210u, 0x0b8310u, 0x208320u, 0x588321u, 0x108410u, 0x258420u, 0x5d8421u, 0x348430u, 0x6c8431u, 0x8f8432u,
    0x148510u, 0x298520u, 0x618521u, 0x388530u, 0x708531u, 0x938532u, 0x428540u, 0x7a8541u, 0x9d8542u, 0xb18543u,
    0x178610u, 0x2c8620u, 0x648621u, 0x3b8630u, 0x738631u, 0x968632u, 0x458640u, 0x7d8641u, 0xa08642u, 0xb48643u,
    0x4b8650u, 0x838651u, 0xa68652u, 0xba8653u, 0xc48654u, 0x198710u, 0x2e8720u, 0x668721u, 0x3d8730u, 0x758731u,
    0x988732u, 0x478740u, 0x7f8741u, 0xa28742u, 0xb68743u, 0x4d8750u, 0x858751u, 0xa88752u, 0xbc8753u, 0xc68754u,
    0x508760u, 0x888761u, 0xab8762u, 0xbf8763u, 0xc98764u, 0xcd8765u, 0x069210u, 0x0c9310u, 0x219320u, 0x599321u,
    0x119410u, 0x269420u, 0x5e9421u, 0x359430u, 0x6d9431u, 0x909432u, 0x159510u, 0x2a9520u, 0x629521u, 0x399530u,
    0x719531u, 0x949532u, 0x439540u, 0x7b9541u, 0x9e9542u, 0xb29543u, 0x189610u, 0x2d9620u, 0x659621u, 0x3c9630u,
    0x749631u, 0x979632u, 0x469640u, 0x7e9641u, 0xa19642u, 0xb59643u, 0x4c9650u, 0x849651u, 0xa79652u, 0xbb9653u,
    0xc59654u, 0x1a9710u, 0x2f9720u, 0x679721u, 0x3e9730u, 0x769731u, 0x999732u, 0x489740u, 0x809741u, 0xa39742u,
    0xb79743u, 0x4e9750u, 0x869751u, 0xa99752u, 0xbd9753u, 0xc79754u, 0x519760u, 0x899761u, 0xac9762u, 0xc09763u,
    0xca9764u, 0xce9765u, 0x1b9810u, 0x309820u, 0x689821u, 0x3f9830u, 0x779831u, 0x9a9832u, 0x499840u, 0x819841u,
    0xa49842u, 0xb89843u, 0x4f9850u, 0x879851u, 0xaa9852u, 0xbe9853u, 0xc89854u, 0x529860u, 0x8a9861u, 0xad9862u,
    0xc19863u, 0xcb9864u, 0xcf9865u, 0x539870u, 0x8b9871u, 0xae9872u, 0xc29873u, 0xcc9874u, 0xd09875u, 0xd19876u,
};
// The ordered pairs of maxima a quad can have as a side, per number of maxima n = 4..10: first the C(n,2) forward pairs
// (a, b), a < b, then the wrapping pairs (d, a) with d - a >= 3 (b and c lie between them); packed first | second<<8.
// kPairOff[n] .. kPairOff[n+1] is n's list: 7, 13, 21, 31, 43, 57, 73 of the n(n-1) ordered pairs.
__device__ const unsigned short kPairOff[12] = {0, 0, 0, 0, 0, 7, 20, 41, 72, 115, 172, 245};
__device__ const unsigned short kPairTab[245] = {
    0x0100, 0x0200, 0x0300, 0x0201, 0x0301, 0x0302, 0x0003, 0x0100, 0x0200, 0x0300, 0x0400, 0x0201, 0x0301, 0x0401,
    0x0302, 0x0402, 0x0403, 0x0003, 0x0004, 0x0104, 0x0100, 0x0200, 0x0300, 0x0400, 0x0500, 0x0201, 0x0301, 0x0401,
    0x0501, 0x0302, 0x0402, 0x0502, 0x0403, 0x0503, 0x0504, 0x0003, 0x0004, 0x0104, 0x0005, 0x0105, 0x0205, 0x0100,
    0x0200, 0x0300, 0x0400, 0x0500, 0x0600, 0x0201, 0x0301, 0x0401, 0x0501, 0x0601, 0x0302, 0x0402, 0x0502, 0x0602,
    0x0403, 0x0503, 0x0603, 0x0504, 0x0604, 0x0605, 0x0003, 0x0004, 0x0104, 0x0005, 0x0105, 0x0205, 0x0006, 0x0106,
    0x0206, 0x0306, 0x0100, 0x0200, 0x0300, 0x0400, 0x0500, 0x0600, 0x0700, 0x0201, 0x0301, 0x0401, 0x0501, 0x0601,
    0x0701, 0x0302, 0x0402, 0x0502, 0x0602, 0x0702, 0x0403, 0x0503, 0x0603, 0x0703, 0x0504, 0x0604, 0x0704, 0x0605,
    0x0705, 0x0706, 0x0003, 0x0004, 0x0104, 0x0005, 0x0105, 0x0205, 0x0006, 0x0106, 0x0206, 0x0306, 0x0007, 0x0107,
    0x0207, 0x0307, 0x0407, 0x0100, 0x0200, 0x0300, 0x0400, 0x0500, 0x0600, 0x0700, 0x0800, 0x0201, 0x0301, 0x0401,
    0x0501, 0x0601, 0x0701, 0x0801, 0x0302, 0x0402, 0x0502, 0x0602, 0x0702, 0x0802, 0x0403, 0x0503, 0x0603, 0x0703,
    0x0803, 0x0504, 0x0604, 0x0704, 0x0804, 0x0605, 0x0705, 0x0805, 0x0706, 0x0806, 0x0807, 0x0003, 0x0004, 0x0104,
    0x0005, 0x0105, 0x0205, 0x0006, 0x0106, 0x0206, 0x0306, 0x0007, 0x0107, 0x0207, 0x0307, 0x0407, 0x0008, 0x0108,
    0x0208, 0x0308, 0x0408, 0x0508, 0x0100, 0x0200, 0x0300, 0x0400, 0x0500, 0x0600, 0x0700, 0x0800, 0x0900, 0x0201,
    0x0301, 0x0401, 0x0501, 0x0601, 0x0701, 0x0801, 0x0901, 0x0302, 0x0402, 0x0502, 0x0602, 0x0702, 0x0802, 0x0902,
    0x0403, 0x0503, 0x0603, 0x0703, 0x0803, 0x0903, 0x0504, 0x0604, 0x0704, 0x0804, 0x0904, 0x0605, 0x0705, 0x0805,
    0x0905, 0x0706, 0x0806, 0x0906, 0x0807, 0x0907, 0x0908, 0x0003, 0x0004, 0x0104, 0x0005, 0x0105, 0x0205, 0x0006,
    0x0106, 0x0206, 0x0306, 0x0007, 0x0107, 0x0207, 0x0307, 0x0407, 0x0008, 0x0108, 0x0208, 0x0308, 0x0408, 0x0508,
    0x0009, 0x0109, 0x0209, 0x0309, 0x0409, 0x0509, 0x0609,
};

struct Moments {
    const double *L[6];  // Mx, My, Mxx, Mxy, Myy, W  (inclusive prefix sums)
    double tot[6];       // L[k][sz - 1], read once per thread and cluster (the kernels are bound by LDS traffic)
    int sz;
};

// gradient weight of a boundary point: sqrt(gx^2 + gy^2) + 1 for the integer n = gx^2 + gy^2 <= 2 * 255^2
#define WEIGHT_TABLE_N (2 * 255 * 255 + 1)
__global__ void __launch_bounds__(256) k_weight_table(double *__restrict__ t)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < WEIGHT_TABLE_N) t[n] = sqrt((double)n) + 1;
}

// moments of the points [i0, i1] of the ordered outline (wrapping when i1 < i0), from the running sums
__device__ __forceinline__ int fit_moments_dev(const Moments &m, int i0, int i1, double (&M)[6])
{
    // One instruction stream for both cases (a wavefront usually holds both): moments of [i0, i1] are L[i1] - L[i0-1]
    // (nothing subtracted for i0 = 0: x - 0.0 is x), and (L[sz-1] - L[i0-1]) + L[i1] for a range that wraps.
    const int sz = m.sz;
    const bool wrap = !(i0 < i1);
    const int N = wrap ? sz - i0 + i1 + 1 : i1 - i0 + 1;
    const bool sub = wrap || i0 > 0;
    const int ib = sub ? i0 - 1 : 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double a = m.L[k][i1], b = sub ? m.L[k][ib] : 0.0, c = m.tot[k];
        const double plain = a - b, wrapped = (c - b) + a;
        M[k] = wrap ? wrapped : plain;
    }
    return N;
}

// line through the points whose moments are M (N of them): centroid, unit normal (lineparm), N * smallest eigenvalue (err), smallest eigenvalue (mse)
// `normal` (only looked at when lineparm is given): false skips the normal -- wave-uniformly when no lane wants it
__device__ __forceinline__ void fit_line_moments_dev(const double (&M)[6], int N, double *lineparm, double *err, double *mse, bool normal = true)
{
    double Mx = M[0], My = M[1], Mxx = M[2], Mxy = M[3], Myy = M[4], W = M[5];
    const Recip rW = recip_of(W);  // five quotients over one denominator (asl_common.h: div_by is a / d bit for bit)
    double Ex = div_by(Mx, rW), Ey = div_by(My, rW);
    double Cxx = div_by(Mxx, rW) - Ex * Ex, Cxy = div_by(Mxy, rW) - Ex * Ey, Cyy = div_by(Myy, rW) - Ey * Ey;
    double disc = (double)sqrtf((float)((Cxx - Cyy) * (Cxx - Cyy) + 4 * Cxy * Cxy));
    double eig_small = 0.5 * (Cxx + Cyy - disc);
    if (lineparm) {
        lineparm[0] = Ex;
        lineparm[1] = Ey;
    }
    if (lineparm && normal) {
        double eig = 0.5 * (Cxx + Cyy + disc);
        double nx1 = Cxx - eig, ny1 = Cxy, M1 = nx1 * nx1 + ny1 * ny1;
        double nx2 = Cxy, ny2 = Cyy - eig, M2 = nx2 * nx2 + ny2 * ny2;
        double nx, ny, MM;
        if (M1 > M2) { nx = nx1; ny = ny1; MM = M1; } else { nx = nx2; ny = ny2; MM = M2; }
        double length = (double)sqrtf((float)MM);
        if (fabs(length) < 1e-12) { lineparm[2] = 0; lineparm[3] = 0; }
        else { const Recip rl = recip_of(length); lineparm[2] = div_by(nx, rl); lineparm[3] = div_by(ny, rl); }
    }
    if (err) *err = N * eig_small;
    if (mse) *mse = eig_small;
}

__device__ __forceinline__ void fit_line_dev(const Moments &m, int i0, int i1, double *lineparm, double *err, double *mse, bool normal = true)
{
    double M[6];
    const int N = fit_moments_dev(m, i0, i1, M);
    fit_line_moments_dev(M, N, lineparm, err, mse, normal);
}

// Ordered compaction over [0,n): for elements with pred(i) true, put(rank, i) with rank = number
// of earlier true elements.  Returns the total.  All NT threads must call it.  One wavefront needs neither LDS nor
// barriers: the running base is a wave-uniform register.
template <int NT, typename Pred, typename Put>
__device__ __forceinline__ int block_compact(int n, int *s_wave, int *s_base, Pred pred, Put put)
{
    constexpr int NW = NT / 64;
    int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (NT == 64) {
        int base = 0;
        for (int start = 0; start < n; start += 64) {
            int i = start + lane;
            bool f = i < n && pred(i);
            unsigned long long mask = __ballot(f);
            if (f) put(base + __popcll(mask & ((1ull << lane) - 1ull)), i);
            base += __popcll(mask);
        }
        return base;
    }
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (int start = 0; start < n; start += NT) {
        int i = start + tid;
        bool f = i < n && pred(i);
        unsigned long long mask = __ballot(f);
        int prefix = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wid] = __popcll(mask);
        __syncthreads();
        int off = *s_base;
        for (int w = 0; w < wid; w++) off += s_wave[w];
        if (f) put(off + prefix, i);
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < NW; w++) tot += s_wave[w];
            *s_base += tot;
        }
        __syncthreads();
    }
    return *s_base;
}

template <int NT, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T ident, T *s_tmp, Op op)
{
    v = wave_scan<true>(v, ident, op);
    if (NT == 64) return v;
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) s_tmp[wid] = v;
    __syncthreads();
    T r = s_tmp[0];
    for (int w = 1; w < NT / 64; w++) r = op(r, s_tmp[w]);
    return r;
}

__device__ __forceinline__ double sqd(double x) { return x * x; }

__device__ __forceinline__ unsigned int float_sortable(float f)
{
    unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- bitonic network over PPT keys per thread, element i = e * NT + tid, with every stride a compile-time constant:
//   stride < 64          partner in the same wavefront: lane_xor<J> (DPP / v_permlane swaps, k_wave.inc), no LDS round trip
//   64 <= stride < NT    partner in another wavefront: one pass through LDS (2 of the 36 stages for 256 keys)
//   stride >= NT         partner is another register of the same thread
// A network is a chain of ~30 dependent exchanges: with ds_bpermute each of them waits for the LDS crossbar.
template <int NT, int PPT, int K, int J>
__device__ __forceinline__ void bitonic_step(unsigned long long (&kr)[PPT], int tid, int npad, unsigned long long *xk)
{
    if constexpr (J >= NT) {
        constexpr int je = J / NT;  // partner register e ^ je
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            if ((e & je) == 0 && (e | je) < PPT) {
                const int eo = e | je;
                if (eo * NT < npad) {  // a register of padding keys only (larger than every real key) stays where it is
                    const bool asc = (((e * NT + tid) & K) == 0);
                    const unsigned long long a = kr[e], b = kr[eo];
                    const bool sw = (a > b) == asc;
                    kr[e] = sw ? b : a;
                    kr[eo] = sw ? a : b;
                }
            }
        }
    } else if constexpr (J >= 64) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PPT; e++) xk[e * NT + tid] = kr[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            const unsigned long long other = xk[e * NT + (tid ^ J)];
            const bool keepmin = ((tid & J) == 0) == (((e * NT + tid) & K) == 0);
            kr[e] = ((kr[e] < other) == keepmin) ? kr[e] : other;
        }
    } else {
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            if (e * NT < npad) {
                const unsigned long long other = lane_xor<J>(kr[e]);
                const bool keepmin = ((tid & J) == 0) == (((e * NT + tid) & K) == 0);
                kr[e] = ((kr[e] < other) == keepmin) ? kr[e] : other;
            }
        }
    }
    if constexpr (J > 1) bitonic_step<NT, PPT, K, J / 2>(kr, tid, npad, xk);
}

template <int NT, int PPT, int K>
__device__ __forceinline__ void bitonic_merge_stages(unsigned long long (&kr)[PPT], int tid, int npad, unsigned long long *xk)
{
    if (K <= npad) bitonic_step<NT, PPT, K, K / 2>(kr, tid, npad, xk);  // npad is the same for all threads of the workgroup
    if constexpr (K < NT * PPT) bitonic_merge_stages<NT, PPT, 2 * K>(kr, tid, npad, xk);
}

// ---- Storage plan.  The steps reach a cluster's arrays only through a FitStore, and only the two functions below build
// one: fit_store_lds for the all-LDS classes (PPT > 0; cap = class capacity in points, R0..R2 = regions of the dynamic
// LDS) and fit_store_slab for the global-slab class (PPT == 0; n = points of the cluster, seg = its n point records,
// S = its 8 n doubles of scratch).  Arrays share memory; "free after" is the barrier that ends an array's lifetime, and no
// array in the same memory is written before it:
//
//   array          all-LDS                      global slab         written   last read            free after
//   keys           R0 [0, 8 cap)                S[0, 2n) as u64     step 1    step 2               the barrier closing step 2
//                  (also the exchange buffer of the sort's cross-wave stages; npad <= cap resp. < 2n keys)
//   xy             R1 [8 cap, 16 cap)           seg as u32          step 2    step 3a              the barrier closing step 3a
//                  (all-LDS: read into registers ahead of step 3a's inner barrier; slab: the point records it overwrites
//                   were read for the last time by step 1)
//   L[0..5]        R2 [16 cap, end), cap + PAD  S[0, 6n), n apart   step 3a   step 6               the barrier opening the
//                  doubles apart                                    step 3b                        next cluster
//                  (slab: over keys)
//   errs           R0 (over keys)               S[6n, 7n)           step 4a   step 4a (low-pass)   the barrier closing step 4a
//   sm             R1 (over xy)                 S[7n, 8n)           step 4a   step 4b (maxima)     the barrier after step 4b's
//                                                                                                  first compaction
//   mx_err         errs[0, sz/2]                the same            step 4b   step 4b (the cut)    the barrier closing step 4b
//   mx_idx         ints from errs + sz/2 + 1    the same            (maxima are never neighbours: at most sz/2 of them)
//   pe, pm         R0 [0, 1600): 2 x 100        static LDS of       step 5    step 5               the barrier opening the
//                  doubles over the maxima      fit_store_slab                                     next cluster
//                  lists; in class 0 (R0 = 1 KB) they run on into R1, over sm
//
// The barrier inside step 3a (all-LDS classes) separates reads of R1 from writes to R2 alone: by this table nothing waits
// for it.  It is kept: removing it would be a change to the kernel, not to its layout.
#define QUAD_LDS_PAD 2                                       /* doubles between the end of one moment array and the next */
#define QUAD_LDS_BYTES(cap) (64 * (cap) + 48 * QUAD_LDS_PAD) /* dynamic LDS of an all-LDS class (launch_fit, aprilslam.hip) */
#define NPAIR (MAX_NMAXIMA * MAX_NMAXIMA)                    /* entries of a pair table of the corner search, [a * MAX_NMAXIMA + b] */

struct FitStore {
    unsigned long long *keys;
    unsigned int *xy;
    double *L0;   // L[k] = L0 + k * lstride
    int lstride;  // all-LDS: the six arrays start 16 bytes apart modulo the bank period, so the six scan lanes never collide
    double *errs, *sm;
    double *pe, *pm;  // pair tables: N * smallest eigenvalue, smallest eigenvalue
    __device__ __forceinline__ double *mx_err() const { return errs; }
    __device__ __forceinline__ int *mx_idx(int sz) const { return reinterpret_cast<int *>(errs + (sz / 2 + 1)); }
};

constexpr size_t fit_lds_r1(int cap) { return 8 * (size_t)cap; }
constexpr size_t fit_lds_r2(int cap) { return 16 * (size_t)cap; }
constexpr int fit_lds_lstride(int cap) { return cap + QUAD_LDS_PAD; }
constexpr size_t fit_lds_end(int cap) { return fit_lds_r2(cap) + 6 * sizeof(double) * fit_lds_lstride(cap); }
static_assert(fit_lds_end(CLASS0_CAP) == QUAD_LDS_BYTES(CLASS0_CAP), "class 0: the plan and the launch disagree about the LDS size");
static_assert(fit_lds_end(CLASS1_CAP) == QUAD_LDS_BYTES(CLASS1_CAP), "class 1: the plan and the launch disagree about the LDS size");
static_assert(fit_lds_end(CLASS2_CAP) == QUAD_LDS_BYTES(CLASS2_CAP), "class 2: the plan and the launch disagree about the LDS size");
static_assert(fit_lds_end(CLASS3_CAP) == QUAD_LDS_BYTES(CLASS3_CAP), "class 3: the plan and the launch disagree about the LDS size");
static_assert(2 * NPAIR * sizeof(double) <= fit_lds_r2(CLASS0_CAP), "the pair tables must end before the moment arrays begin");

__device__ __forceinline__ FitStore fit_store_lds(unsigned char *smem, int cap)
{
    FitStore st;
    st.keys = reinterpret_cast<unsigned long long *>(smem);
    st.xy = reinterpret_cast<unsigned int *>(smem + fit_lds_r1(cap));
    st.L0 = reinterpret_cast<double *>(smem + fit_lds_r2(cap));
    st.lstride = fit_lds_lstride(cap);
    st.errs = reinterpret_cast<double *>(smem);
    st.sm = reinterpret_cast<double *>(smem + fit_lds_r1(cap));
    st.pe = reinterpret_cast<double *>(smem);
    st.pm = reinterpret_cast<double *>(smem) + NPAIR;
    return st;
}

__device__ __forceinline__ FitStore fit_store_slab(unsigned long long *seg, double *S, int n)
{
    __shared__ double s_pe[NPAIR], s_pm[NPAIR];
    FitStore st;
    st.keys = reinterpret_cast<unsigned long long *>(S);
    st.xy = reinterpret_cast<unsigned int *>(seg);
    st.L0 = S;
    st.lstride = n;
    st.errs = S + (size_t)6 * n;
    st.sm = S + (size_t)7 * n;
    st.pe = s_pe;
    st.pm = s_pm;
    return st;
}

// The workgroup's static LDS: separate variables of k_fit_quads, not one struct, so that an instantiation holds only those
// it uses (one wavefront needs no cross-wave scratch) -- every static byte counts: at 10 KB per workgroup a CU holds 16 of
// them.  Nothing here shares memory with anything else.
struct FitShared {
    int *wave, *base;                    // block_compact's cross-wave scratch
    int *tmpi; long long *tmpl; double *tmpd;  // block_reduce's, one per type
    int *maxidx;                         // the (at most MAX_NMAXIMA) maxima: step 4b -> step 5
    double *pnx, *pny;                   // pair tables of step 5: unit normal of a forward pair's line
    int *found, *best; double *thresh;   // step 5's verdict: a winner exists, its four maxima (-> step 6), its total error
};

// ---- Fetch of this workgroup's clusters li = blockIdx.x, blockIdx.x + G, ... (G = gridDim.x) of the class list.
// All-LDS classes: a software pipeline.  The three dependent fetches that open a cluster (list entry -> cluster record ->
// point records, PPT per thread) are issued three, two and one clusters ahead, so their latency hides behind the
// arithmetic of the clusters in between.  List indices past the end are clamped to the last entry, not guarded: the tail
// fetches the last cluster again and nobody looks at it.  Global-slab class: the plain two loads (the steps read the
// point records from memory).
template <int NT, int PPT>
struct FitFetch {
    static constexpr int NREC = PPT > 0 ? PPT : 1;
    const unsigned int *class_list;
    const ClusterRec *clusters;
    const unsigned long long *points;
    unsigned int last;  // index of the class list's last entry
    unsigned int ci_nx, ci_nn, ci_n3;
    ClusterRec cl_nx, cl_nn;
    unsigned long long recs_nx[NREC];

    __device__ __forceinline__ void load_recs()
    {
        const int tid = threadIdx.x;
#pragma unroll
        for (int e = 0; e < NREC; e++) {
            int i = tid + e * NT;
            recs_nx[e] = i < (int)cl_nx.count ? points[(size_t)cl_nx.offset + i] : 0ull;
        }
    }
    // before the loop; ncl > blockIdx.x
    __device__ __forceinline__ void open(const unsigned int *class_list_, const ClusterRec *clusters_, const unsigned long long *points_, unsigned int ncl)
    {
        class_list = class_list_; clusters = clusters_; points = points_; last = ncl - 1;
        if constexpr (PPT > 0) {
            const unsigned int G = gridDim.x;
            ci_nx = class_list[blockIdx.x];
            ci_nn = class_list[min(blockIdx.x + G, last)];
            ci_n3 = class_list[min(blockIdx.x + 2 * G, last)];
            cl_nx = clusters[ci_nx];
            cl_nn = clusters[ci_nn];
            load_recs();
        }
    }
    // once per iteration: hands out cluster li (its index, its record and, PPT > 0, this thread's point records) and refills
    __device__ __forceinline__ void advance(unsigned int li, unsigned int &ci, ClusterRec &cl, unsigned long long (&recs)[NREC])
    {
        if constexpr (PPT > 0) {
            ci = ci_nx; cl = cl_nx;
#pragma unroll
            for (int e = 0; e < NREC; e++) recs[e] = recs_nx[e];
            ci_nx = ci_nn; cl_nx = cl_nn;
            load_recs();
            ci_nn = ci_n3;
            cl_nn = clusters[ci_nn];
            ci_n3 = class_list[min(li + 3 * gridDim.x, last)];
        } else {
            ci = class_list[li];
            cl = clusters[ci];
        }
    }
};

// ---- The steps.  Each header says what the step reads and writes (FitStore / FitShared members), whether it ends with a
// barrier, and who must call it.  "Every thread": all NT threads of the workgroup, in uniform control flow.  A value a step
// returns is the same in every thread.

// Step 0: bounding box, gradient sums, polarity.  Reads the cluster's n point records (PPT > 0: recs, this thread's,
// fetched ahead; else seg); writes sh.tmpi, sh.tmpl.  Gives the box centre (cx, cy) and returns the border polarity
// (1 = reversed), or -1 = reject (box smaller than a tag, or a polarity nobody wants).  No closing barrier (the reductions
// hold their own).  Every thread.
template <int NT, int PPT>
__device__ __forceinline__ int fit_box_polarity(const FitShared &sh, const unsigned long long (&recs)[PPT > 0 ? PPT : 1], const unsigned long long *seg, int n,
                                                 int tag_width, int want_reversed, int want_normal, float &cx, float &cy)
{
    const int tid = threadIdx.x;
    int xmin = 0x7FFFFFFF, xmax = 0, ymin = 0x7FFFFFFF, ymax = 0, sgx = 0, sgy = 0;
    long long sxg = 0;
    auto accumulate = [&](unsigned long long r) {
        int px = (int)(r & 0xFFFFu), py = (int)((r >> 16) & 0xFFFFu);
        int cgx = (int)((r >> 32) & 3u), cgy = (int)((r >> 34) & 3u);
        int gx = cgx == 0 ? 0 : (cgx == 1 ? 255 : -255), gy = cgy == 0 ? 0 : (cgy == 1 ? 255 : -255);
        xmin = min(xmin, px); xmax = max(xmax, px); ymin = min(ymin, py); ymax = max(ymax, py);
        sgx += gx; sgy += gy;
        sxg += (long long)(px * gx + py * gy);
    };
    if constexpr (PPT > 0) {
#pragma unroll
        for (int e = 0; e < PPT; e++)
            if (tid + e * NT < n) accumulate(recs[e]);
    } else {
        for (int i = tid; i < n; i += NT) accumulate(seg[i]);
    }
    xmin = block_reduce<NT>(xmin, 0x7FFFFFFF, sh.tmpi, [](int a, int b) { return a < b ? a : b; });
    xmax = block_reduce<NT>(xmax, 0, sh.tmpi, [](int a, int b) { return a > b ? a : b; });
    ymin = block_reduce<NT>(ymin, 0x7FFFFFFF, sh.tmpi, [](int a, int b) { return a < b ? a : b; });
    ymax = block_reduce<NT>(ymax, 0, sh.tmpi, [](int a, int b) { return a > b ? a : b; });
    sgx = block_reduce<NT>(sgx, 0, sh.tmpi, [](int a, int b) { return a + b; });
    sgy = block_reduce<NT>(sgy, 0, sh.tmpi, [](int a, int b) { return a + b; });
    sxg = block_reduce<NT>(sxg, 0ll, sh.tmpl, [](long long a, long long b) { return a + b; });
    if ((xmax - xmin) * (ymax - ymin) < tag_width) return -1;
    cx = (float)((double)(xmin + xmax) * 0.5 + 0.05118);
    cy = (float)((double)(ymin + ymax) * 0.5 + -0.028581);
    // dot = sum (x-cx)*gx + (y-cy)*gy evaluated from exact integer sums
    double dot = (double)sxg - (double)cx * (double)sgx - (double)cy * (double)sgy;
    const int reversed = dot < 0 ? 1 : 0;
    return ((reversed && !want_reversed) || (!reversed && !want_normal)) ? -1 : reversed;
}

// Step 1: sort keys and bitonic sort.  Reads the point records (as step 0); writes st.keys[0, npad), npad = n rounded up to
// a power of two, at least 64 (padding keys are ~0), sorted.  Ends with a barrier.  Every thread.
template <int NT, int PPT>
__device__ __forceinline__ void fit_sort_keys(const FitStore &st, const unsigned long long (&recs)[PPT > 0 ? PPT : 1], const unsigned long long *seg, int n,
                                              float cx, float cy)
{
    const int tid = threadIdx.x;
    unsigned long long *const keys = st.keys;
    int npad = 64;
    while (npad < n) npad <<= 1;
    auto make_key = [&](unsigned long long r) -> unsigned long long {
        int px = (int)(r & 0xFFFFu), py = (int)((r >> 16) & 0xFFFFu);
        // angle key about the box centre (monotone in the angle, no trig): quadrant + dy/dx
        float dx = (float)px - cx, dy = (float)py - cy;
        float quadrant = (dy > 0) ? ((dx > 0) ? 65536.0f : 131072.0f) : ((dx > 0) ? 0.0f : -65536.0f);
        if (dy < 0) { dy = -dy; dx = -dx; }
        if (dx < 0) { float t = dx; dx = dy; dy = -t; }
        float slope = quadrant + dy / dx;
        return ((unsigned long long)float_sortable(slope) << 32) | (r & 0xFFFFFFFFull);
    };
    if constexpr (PPT > 0) {
        // PPT keys per thread (element i = e * NT + tid): the whole network runs in registers (bitonic_step above) and the
        // sorted keys are written to LDS once
        unsigned long long kr[PPT];
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            int i = tid + e * NT;
            kr[e] = i < n ? make_key(recs[e]) : ~0ull;
        }
        bitonic_merge_stages<NT, PPT, 2>(kr, tid, NT == 64 ? npad : NT * PPT, keys);
        if (NT > 64) __syncthreads();  // keys was the exchange buffer
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            int i = tid + e * NT;
            if (i < npad) keys[i] = kr[e];
        }
        __syncthreads();
    } else {
        for (int i = tid; i < npad; i += NT) keys[i] = i < n ? make_key(seg[i]) : ~0ull;
        __syncthreads();
        for (int k = 2; k <= npad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npad; i += NT) {
                    int ixj = i ^ j;
                    if (ixj > i) {
                        unsigned long long a = keys[i], b = keys[ixj];
                        bool asc = (i & k) == 0;
                        if ((a > b) == asc) { keys[i] = b; keys[ixj] = a; }
                    }
                }
                __syncthreads();
            }
    }
}

// Step 2: drop duplicate points (same x,y are adjacent after the sort).  Reads st.keys[0, n); writes st.xy[0, sz), sh.wave,
// sh.base.  Gives sz, the number of distinct points.  Ends with a barrier.  Every thread.
template <int NT>
__device__ __forceinline__ int fit_dedup(const FitStore &st, const FitShared &sh, int n)
{
    const unsigned long long *const keys = st.keys;
    unsigned int *const xy = st.xy;
    int sz = block_compact<NT>(
        n, sh.wave, sh.base,
        [&](int i) { return i == 0 || (unsigned int)keys[i] != (unsigned int)keys[i - 1]; },
        [&](int rank, int i) { xy[rank] = (unsigned int)keys[i]; });
    __syncthreads();
    return sz;
}

// Step 3a: every point's six terms W*x, W*y, W*x*x, W*x*y, W*y*y, W (W = gradient weight from the frame im), computed by
// all lanes.  Reads st.xy[0, sz); writes L[0..5][0, sz).  Ends with a barrier.  Every thread.
template <int NT, int PPT>
__device__ __forceinline__ void fit_terms(const FitStore &st, int sz, const uint8_t *im, const Geom &g, const double *__restrict__ wtab)
{
    const int tid = threadIdx.x;
    const unsigned int *const xy = st.xy;
    double *const L0 = st.L0;
    const int lstride = st.lstride;
    auto put_terms = [&](int i, unsigned int v) {
        double x = (double)(v & 0xFFFFu) * .5 + 0.5, y = (double)(v >> 16) * .5 + 0.5;
        int ix = (int)x, iy = (int)y;
        double W = 1;
        if (ix > 0 && ix + 1 < g.sw && iy > 0 && iy + 1 < g.sh) {
            int grad_x = (int)im[iy * g.sw + ix + 1] - (int)im[iy * g.sw + ix - 1];
            int grad_y = (int)im[(iy + 1) * g.sw + ix] - (int)im[(iy - 1) * g.sw + ix];
            W = wtab[grad_x * grad_x + grad_y * grad_y];  // sqrt(n) + 1, tabulated (k_weight_table): one gather instead of a double-precision square root
        }
        L0[i] = W * x;
        L0[(size_t)lstride + i] = W * y;
        L0[(size_t)2 * lstride + i] = W * x * x;
        L0[(size_t)3 * lstride + i] = W * x * y;
        L0[(size_t)4 * lstride + i] = W * y * y;
        L0[(size_t)5 * lstride + i] = W;
    };
    if constexpr (PPT > 0) {
        // unrolled so that the gradient gathers of all of this thread's points are in flight together
        unsigned int pv[PPT];
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            int i = tid + e * NT;
            pv[e] = i < sz ? xy[i] : 0u;
        }
        __syncthreads();  // see the storage plan: kept, though nothing waits for it
#pragma unroll
        for (int e = 0; e < PPT; e++) {
            int i = tid + e * NT;
            if (i < sz) put_terms(i, pv[e]);
        }
    } else {
        for (int i = tid; i < sz; i += NT) put_terms(i, xy[i]);
    }
    __syncthreads();
}

// Step 3b: the ordered (sequential, bit-exact) part: a bare running sum per array, one lane each.  Reads and writes
// L[0..5][0, sz) in place.  Gives the Moments every later step reads L through.  Ends with a barrier.  Every thread.
__device__ __forceinline__ Moments fit_running_sums(const FitStore &st, int sz)
{
    const int tid = threadIdx.x;
    if (tid < 6) {
        double acc = 0;
        double *out = st.L0 + (size_t)tid * st.lstride;
#pragma unroll 8
        for (int i = 0; i < sz; i++) {
            acc += out[i];
            out[i] = acc;
        }
    }
    __syncthreads();
    Moments mom;
    for (int k = 0; k < 6; k++) { mom.L[k] = st.L0 + (size_t)k * st.lstride; mom.tot[k] = mom.L[k][sz - 1]; }
    mom.sz = sz;
    return mom;
}

// Step 4a: line-fit error of the window [i - ksz, i + ksz] about every point, then the 7-tap low-pass.  Reads L; writes
// st.errs[0, sz), then st.sm[0, sz).  Ends with a barrier.  Every thread.
template <int NT>
__device__ __forceinline__ void fit_window_errors(const FitStore &st, const Moments &mom, int ksz)
{
    const float LPF[7] = {0.011108996538242306f, 0.1353352832366127f, 0.6065306597126334f, 1.0f,
                          0.6065306597126334f, 0.1353352832366127f, 0.011108996538242306f};
    const int tid = threadIdx.x, sz = mom.sz;
    double *const errs = st.errs, *const sm = st.sm;
    for (int i = tid; i < sz; i += NT) {
        double e;
        int i0 = i - ksz, i1 = i + ksz;
        if (i0 < 0) i0 += sz;
        if (i1 >= sz) i1 -= sz;
        fit_line_dev(mom, i0, i1, nullptr, &e, nullptr);
        errs[i] = e;
    }
    __syncthreads();
    for (int i = tid; i < sz; i += NT) {
        double acc = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            int t = i + k - 3;
            if (t < 0) t += sz;
            if (t >= sz) t -= sz;
            acc += errs[t] * LPF[k];
        }
        sm[i] = acc;
    }
    __syncthreads();
}

// Step 4b: the local maxima of the smoothed error, in outline order, cut to the MAX_NMAXIMA strongest.  Reads st.sm[0, sz);
// writes the maxima lists st.mx_err(), st.mx_idx(sz), then sh.maxidx[0, nmax); also sh.wave, sh.base, sh.thresh.  Gives
// nmax; fewer than 4 = reject (sh.maxidx is then not written).  Ends with a barrier.  Every thread.
template <int NT>
__device__ __forceinline__ int fit_maxima(const FitStore &st, const FitShared &sh, int sz)
{
    const int tid = threadIdx.x;
    const double *const sm = st.sm;
    double *const mx_err = st.mx_err();
    int *const mx_idx = st.mx_idx(sz);
    int nmax = block_compact<NT>(
        sz, sh.wave, sh.base, [&](int i) { return sm[i] > sm[i + 1 == sz ? 0 : i + 1] && sm[i] > sm[i == 0 ? sz - 1 : i - 1]; },
        [&](int rank, int i) { mx_err[rank] = sm[i]; mx_idx[rank] = i; });
    __syncthreads();
    if (nmax < 4) return nmax;
    if (nmax > MAX_NMAXIMA) {
        // threshold = the (MAX_NMAXIMA+1)-th largest error; keep strictly larger ones, in order
        for (int j = tid; j < nmax; j += NT) {
            double e = mx_err[j];
            int gt = 0, ge = 0;
            for (int k = 0; k < nmax; k++) { double o = mx_err[k]; gt += o > e; ge += o >= e; }
            if (gt <= MAX_NMAXIMA && MAX_NMAXIMA < ge) *sh.thresh = e;  // every writer writes the same value
        }
        __syncthreads();
        double thr = *sh.thresh;
        int kept = block_compact<NT>(
            nmax, sh.wave, sh.base, [&](int j) { return mx_err[j] > thr; },
            [&](int rank, int j) { if (rank < MAX_NMAXIMA) sh.maxidx[rank] = mx_idx[j]; });
        __syncthreads();
        nmax = kept < MAX_NMAXIMA ? kept : MAX_NMAXIMA;
    } else {
        if (tid < nmax) sh.maxidx[tid] = mx_idx[tid];
        __syncthreads();
    }
    return nmax;
}

// Step 5: best 4 of nmax <= 10 maxima.  Every candidate side is one of the nmax*(nmax-1) ordered pairs of maxima, so the
// line fits are done once per pair (in lockstep across lanes) and the C(nmax,4) combinations only add table entries -- same
// values, same order of additions.  Reads L, sh.maxidx; writes the pair tables st.pe, st.pm, sh.pnx, sh.pny, then sh.found,
// sh.best[0, 4), sh.thresh; also sh.tmpd, sh.tmpi.  True = a combination passed and its mean error is small enough (sh.best
// holds its maxima).  Ends with a barrier.  Every thread.
template <int NT>
__device__ __forceinline__ bool fit_corner_search(const FitStore &st, const FitShared &sh, const Moments &mom, int nmax)
{
    const int tid = threadIdx.x;
    double *const s_pe = st.pe, *const s_pm = st.pm, *const s_pnx = sh.pnx, *const s_pny = sh.pny;
    const int *const s_maxidx = sh.maxidx;
    // only the pairs a quad can use (kPairTab: 73 of the 90 for ten maxima, 57 of 72 for nine: one round of 64 lanes
    // less), forward pairs first: the normals are wanted of those alone (the angle test is between the sides
    // (a,b) and (b,c)), so a round of wrapping pairs skips them
    const int pair0 = kPairOff[nmax], npairs = kPairOff[nmax + 1] - pair0;
    for (int p = tid; p < npairs; p += NT) {
        const unsigned int pr = kPairTab[pair0 + p];
        const int a = (int)(pr & 0xFFu), b = (int)(pr >> 8);
        double prm[4], e, m;
        fit_line_dev(mom, s_maxidx[a], s_maxidx[b], prm, &e, &m, a < b);
        s_pe[a * MAX_NMAXIMA + b] = e; s_pm[a * MAX_NMAXIMA + b] = m;
        if (a < b) { s_pnx[a * MAX_NMAXIMA + b] = prm[2]; s_pny[a * MAX_NMAXIMA + b] = prm[3]; }
    }
    __syncthreads();
    double myerr = HUGE_VAL;
    int myrank = 0x7FFFFFFF, mine[4] = {0, 0, 0, 0};
    const int ncombo = nmax * (nmax - 1) * (nmax - 2) * (nmax - 3) / 24;  // the subsets of {0..nmax-1} lead the table
    for (int k = tid; k < ncombo; k += NT) {
        const unsigned int cmb = kCombo4of10[k];
        const int a = cmb & 15u, b = (cmb >> 4) & 15u, c = (cmb >> 8) & 15u, d = (cmb >> 12) & 15u, rank = (int)(cmb >> 16);
        int ab = a * MAX_NMAXIMA + b, bc = b * MAX_NMAXIMA + c, cd = c * MAX_NMAXIMA + d, da = d * MAX_NMAXIMA + a;
        if (s_pm[ab] > MAX_LINE_FIT_MSE) continue;
        if (s_pm[bc] > MAX_LINE_FIT_MSE) continue;
        double dt = s_pnx[ab] * s_pnx[bc] + s_pny[ab] * s_pny[bc];
        if (fabs(dt) > COS_CRITICAL_RAD) continue;
        if (s_pm[cd] > MAX_LINE_FIT_MSE) continue;
        if (s_pm[da] > MAX_LINE_FIT_MSE) continue;
        double e = s_pe[ab] + s_pe[bc] + s_pe[cd] + s_pe[da];
        if (e < myerr || (e == myerr && rank < myrank)) { myerr = e; myrank = rank; mine[0] = s_maxidx[a]; mine[1] = s_maxidx[b]; mine[2] = s_maxidx[c]; mine[3] = s_maxidx[d]; }
    }
    double best = block_reduce<NT>(myerr, (double)HUGE_VAL, sh.tmpd, [](double a, double b) { return a < b ? a : b; });
    // among equal errors the combination that comes first in lexicographic order wins (upstream's strict '<' in its loop order)
    int cand = (myerr == best && myerr < (double)HUGE_VALF) ? myrank : 0x7FFFFFFF;
    int brank = block_reduce<NT>(cand, 0x7FFFFFFF, sh.tmpi, [](int a, int b) { return a < b ? a : b; });
    if (tid == 0) *sh.found = 0;
    __syncthreads();
    if (brank != 0x7FFFFFFF && cand == brank) {
        *sh.found = 1;
        for (int k = 0; k < 4; k++) sh.best[k] = mine[k];
        *sh.thresh = best;
    }
    __syncthreads();
    return *sh.found && *sh.thresh / mom.sz < MAX_LINE_FIT_MSE;
}

// Step 6: the four sides of the best combination: only their moments are gathered here.  The line fits, corners and sanity
// checks are a serial double-precision chain with four independent items per cluster: k_quad_finish runs them with four
// lanes per cluster, sixteen clusters per wavefront (as the tail of this kernel they were an eighth of its instructions,
// issued for 64 or 128 lanes with four at work).  Reads L, sh.best; writes cluster ci's 4 x 6 doubles of side_mom (global).
// No barrier; threads 0..3 work, any thread may call.
__device__ __forceinline__ void fit_side_moments(const FitShared &sh, const Moments &mom, double *side_mom, unsigned int ci)
{
    const int tid = threadIdx.x, sz = mom.sz;
    if (tid < 4) {
        // a sixth of the side is left out at either end: the points next to a corner are the least reliable
        // ones; the reference's committed run only reproduces with this on (tests/golden/README.md)
        int i0 = sh.best[tid], i1 = sh.best[(tid + 1) & 3];
        int len = i1 - i0;
        if (len < 0) len += sz;
        if (len > 8) {
            int t = len / 6;
            i0 = (i0 + t) % sz;
            i1 = (i1 + sz - t) % sz;
        }
        double M[6];
        fit_moments_dev(mom, i0, i1, M);
        double *out = side_mom + ((size_t)ci * 4 + tid) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) out[k] = M[k];
    }
}

// One workgroup per cluster at a time, grid-stride over the class's list.  PPT = class capacity / NT (points per thread) for
// the all-LDS classes (the sort network runs in registers), 0 for the global-slab class.  A rejected cluster leaves the
// loop body at once (every reject is the same in all threads); its quad stays invalid.  valid = 2: waiting for k_quad_finish.
template <int NT, int PPT>
__global__ void __launch_bounds__(NT) k_fit_quads(const ClusterRec *__restrict__ clusters, const unsigned int *__restrict__ class_list,
                                                  const long long *__restrict__ counters, int cls, unsigned int max_clusters, int cap,
                                                  unsigned long long *points, const uint8_t *__restrict__ dgray, Geom g, int tag_width,
                                                  int want_reversed, int want_normal, double *scratch, QuadRec *quads, const double *__restrict__ wtab,
                                                  double *__restrict__ side_mom)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_wave[4], s_base, s_n;
    __shared__ int s_maxidx[MAX_NMAXIMA], s_best[4];
    __shared__ double s_thresh;
    __shared__ double s_tmpd[4];
    __shared__ long long s_tmpl[4];
    __shared__ int s_tmpi[4];
    __shared__ double s_pnx[NPAIR], s_pny[NPAIR];
    const FitShared sh = {s_wave, &s_base, s_tmpi, s_tmpl, s_tmpd, s_maxidx, s_pnx, s_pny, &s_n, s_best, &s_thresh};
    const int tid = threadIdx.x;
    PHASE_DECL();
    if (batch_poisoned(counters)) return;
    long long ncl64 = counters[CNT_CLASS(cls)];
    unsigned int ncl = ncl64 > (long long)max_clusters ? max_clusters : (unsigned int)ncl64;
    if (blockIdx.x >= ncl) return;
    FitFetch<NT, PPT> fetch;
    fetch.open(class_list, clusters, points, ncl);

    for (unsigned int li = blockIdx.x; li < ncl; li += gridDim.x) {
        __syncthreads();  // previous iteration's shared state is dead
        PHASE_INIT();
        unsigned int ci;
        ClusterRec cl;
        unsigned long long recs[FitFetch<NT, PPT>::NREC];
        fetch.advance(li, ci, cl, recs);
        if (tid == 0) { quads[ci].valid = 0; quads[ci].key = cl.key; quads[ci].reversed_border = 0; }
        const int n = (int)cl.count;
        if (n < 24) continue;
        unsigned long long *seg = points + cl.offset;
        FitStore st;
        if constexpr (PPT > 0) st = fit_store_lds(smem, cap);
        else st = fit_store_slab(seg, scratch + (size_t)cl.offset * 8, n);  // 8 doubles per point

        float cx, cy;
        const int reversed = fit_box_polarity<NT, PPT>(sh, recs, seg, n, tag_width, want_reversed, want_normal, cx, cy);
        if (reversed < 0) continue;
        if (tid == 0) quads[ci].reversed_border = reversed;
        PHASE(0);
        fit_sort_keys<NT, PPT>(st, recs, seg, n, cx, cy);
        const int sz = fit_dedup<NT>(st, sh, n);
        if (sz < 24) continue;
        PHASE(2);
        fit_terms<NT, PPT>(st, sz, dgray + (size_t)(int)(cl.key >> 48) * g.npix, g, wtab);
        PHASE(3);
        const Moments mom = fit_running_sums(st, sz);
        PHASE(4);
        const int ksz = sz / 12 < 20 ? sz / 12 : 20;
        if (ksz < 2) continue;
        fit_window_errors<NT>(st, mom, ksz);
        PHASE(5);
        const int nmax = fit_maxima<NT>(st, sh, sz);
        if (nmax < 4) continue;
        PHASE(6);
        const bool won = fit_corner_search<NT>(st, sh, mom, nmax);
        PHASE(7);
        if (!won) continue;
        fit_side_moments(sh, mom, side_mom, ci);
        if (tid == 0) quads[ci].valid = 2;
        PHASE(8);
    }
    PHASE_FLUSH(0);
}

// Final lines, corners and sanity checks of the clusters the fit kernels left with valid = 2: FOUR LANES PER CLUSTER (lane l
// = side l and corner l), sixteen clusters per wavefront.  Identical arithmetic per item as the scalar formulation (line of
// side l from its moments; corner l = intersection of sides l and l+1; Heron's formula for the triangles (0,1,2) by lane 0
// and (2,3,0) by lane 1, added in that order; the angle at corner l+1); neighbours' values come through DPP quad
// permutations.  A cluster that fails a check is computed to the end like the others (no lane leaves; infinities and NaNs of
// a degenerate cluster stay in its four lanes) and is marked invalid.
__global__ void __launch_bounds__(256) k_quad_finish(QuadRec *__restrict__ quads, const double *__restrict__ side_mom, const long long *__restrict__ counters,
                                                     unsigned int max_clusters, int tag_width)
{
    if (batch_poisoned(counters)) return;
    const long long ncl64 = counters[CNT_NCLUSTERS];
    const unsigned int ncl = ncl64 > (long long)max_clusters ? max_clusters : (unsigned int)ncl64;
    const int lane = threadIdx.x & 63, l = lane & 3;
    for (unsigned int c0 = blockIdx.x * 64u; c0 < ncl; c0 += gridDim.x * 64u) {
        const unsigned int ci = c0 + (threadIdx.x >> 2);
        const bool pending = ci < ncl && quads[ci].valid == 2;
        if (!__any(pending)) continue;  // wave-uniform
        double M[6];
        const double *in = side_mom + ((size_t)(pending ? ci : 0) * 4 + l) * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) M[k] = pending ? in[k] : 1.0;
        double line[4], mse;
        fit_line_moments_dev(M, 0, line, nullptr, &mse);
        bool fail = mse > MAX_LINE_FIT_MSE;
        // corner l: sides l and l + 1
        const double n0 = dpp_mov<QUAD_ROT1>(0.0, line[0]), n1 = dpp_mov<QUAD_ROT1>(0.0, line[1]), n2 = dpp_mov<QUAD_ROT1>(0.0, line[2]), n3 = dpp_mov<QUAD_ROT1>(0.0, line[3]);
        const double A00 = line[3], A01 = -n3;
        const double A10 = -line[2], A11 = n2;
        const double B0 = -line[0] + n0;
        const double B1 = -line[1] + n1;
        const double det = A00 * A11 - A10 * A01;
        double Px = 0, Py = 0;
        if (fabs(det) < 0.001) fail = true;
        else {
            const double W00 = A11 / det, W01 = -A01 / det;
            const double L0v = W00 * B0 + W01 * B1;
            Px = line[0] + L0v * A00;
            Py = line[1] + L0v * A10;
        }
        const double P1x = dpp_mov<QUAD_ROT1>(0.0, Px), P1y = dpp_mov<QUAD_ROT1>(0.0, Py), P2x = dpp_mov<QUAD_ROT2>(0.0, Px), P2y = dpp_mov<QUAD_ROT2>(0.0, Py);
        const double P3x = dpp_mov<QUAD_ROT3>(0.0, Px), P3y = dpp_mov<QUAD_ROT3>(0.0, Py);
        // triangles (0,1,2) in lane 0 and (2,3,0) in lane 1: the vertices are this lane's corners l, l+1, l+2 resp. l+1, l+2, l+3
        const bool t0 = l == 0;
        const double ax = t0 ? Px : P1x, ay = t0 ? Py : P1y, bx = t0 ? P1x : P2x, by = t0 ? P1y : P2y, cx = t0 ? P2x : P3x, cy = t0 ? P2y : P3y;
        const double len0 = sqrt(sqd(bx - ax) + sqd(by - ay)), len1 = sqrt(sqd(cx - bx) + sqd(cy - by)), len2 = sqrt(sqd(ax - cx) + sqd(ay - cy));
        const double p = (len0 + len1 + len2) / 2;
        const double tri = sqrt(p * (p - len0) * (p - len1) * (p - len2));
        // angle at corner l + 1 between the sides (l, l+1) and (l+1, l+2), and the winding
        const double dx1 = P1x - Px, dy1 = P1y - Py;
        const double dx2 = P2x - P1x, dy2 = P2y - P1y;
        const double cos_dtheta = (dx1 * dx2 + dy1 * dy2) / sqrt((dx1 * dx1 + dy1 * dy1) * (dx2 * dx2 + dy2 * dy2));
        if ((cos_dtheta > COS_CRITICAL_RAD || cos_dtheta < -COS_CRITICAL_RAD) || dx1 * dy2 < dy1 * dx2) fail = true;
        const bool any_fail = ((__ballot(fail) >> (lane & ~3)) & 0xFull) != 0;
        double area = 0;
        area += tri;                           // lane 0: s_tri[0]
        area += dpp_mov<QUAD_ROT1>(0.0, tri);  // lane 0: + s_tri[1]
        if (pending) {
            quads[ci].p[l][0] = Px; quads[ci].p[l][1] = Py;
            if (l == 0) quads[ci].valid = (!any_fail && !(area < 0.95 * tag_width * tag_width)) ? 1 : 0;
        }
    }
}

// Not every cluster yields a quad (107 of 186 per frame in the bench scene).  The refine/decode kernels walk this compact list of survivors instead of
// all clusters; allocation is aggregated per 1024-thread block (one global atomic per block -- a single address
// sustains only ~90 atomics/us, so appending from the fit kernels themselves would cost more than it saves).
__global__ void __launch_bounds__(1024) k_quad_compact(const QuadRec *__restrict__ quads, long long *counters, unsigned int max_clusters,
                                                       unsigned int *__restrict__ quad_list)
{
    __shared__ unsigned int s_cnt[16];
    __shared__ unsigned long long s_base;
    if (batch_poisoned(counters)) return;
    long long ncl64 = counters[CNT_NCLUSTERS];
    unsigned int ncl = ncl64 > (long long)max_clusters ? max_clusters : (unsigned int)ncl64;
    if (blockIdx.x * blockDim.x >= ncl) return;
    unsigned int ci = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    bool keep = ci < ncl && quads[ci].valid != 0;
    unsigned long long m = __ballot(keep);
    if (lane == 0) s_cnt[wid] = (unsigned int)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int w = 0; w < 16; w++) t += s_cnt[w];
        s_base = t ? atomicAdd((unsigned long long *)&counters[CNT_NQUADS], (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    if (!keep) return;
    unsigned long long at = s_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; w++) at += s_cnt[w];
    quad_list[at] = ci;
}
