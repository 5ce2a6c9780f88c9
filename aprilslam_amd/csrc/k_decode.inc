// S7: bit decoding and code-book match (k_decode), from the homography k_homography left (k_refine.inc).  One wavefront
// per candidate quad: lanes take the independent samples (border samples, the payload bits, the buckets of the code-book
// index), designated lanes do the small ordered reductions so that every float sum has the same order as a scalar loop.
// The full-resolution gray value is computed on demand from the BGR frame (gray_at).

__device__ __forceinline__ void hproject_dev(const double *H, double x, double y, double *ox, double *oy)
{
    double xx = H[0] * x + H[1] * y + H[2];
    double yy = H[3] * x + H[4] * y + H[5];
    double zz = H[6] * x + H[7] * y + H[8];
    *ox = xx / zz;
    *oy = yy / zz;
}

struct GrayModel { double A[9], B[3], C[3]; };

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

// ---- Storage plan of k_decode: the workgroup's LDS, one wavefront.  The kernel holds one DecodeStore; the steps reach it
// only through their argument.  Nothing shares memory.  The capacities are what the store assumes of a family:
#define DEC_BORDER_CAP 64 /* border samples, 8 patterns of width_at_border each, one lane each: width_at_border <= 8 */
#define DEC_GRID_CAP 16   /* cells along a side of the payload grid: total_width <= 16 */
#define DEC_BITS_CAP 64   /* payload bits, one lane each: nbits <= 64 */
// A family beyond these is refused when the detector is made (asl_family_check), never truncated here.
// Barriers of a quad: L opens it (loop top), A follows H, B the border samples, C the gray models, D the payload values,
// E (inside decode_scores) the two lists.
//
//   member      bytes   holds                          written by                     read by                       free after
//   smpxy       1024    tag-frame coordinates of the   tag_sites, once per            border_samples,               never: constant for the
//   bitxy       1024    border samples / payload bits  workgroup, ahead of the        payload_values                workgroup's life
//                                                      first L
//   H           72      the quad's homography          the body: lanes 0-8            border_samples,               L of the next quad
//                                                                                     payload_values (behind A),
//                                                                                     emit
//   smp         2048    border rows (x, y, gray, 1),   border_samples: the sample's   gray_models: lanes 0-17       L of the next quad
//                       zeros for a sample outside     lane                           (behind B)
//   white,      240     the two gray models            gray_models: lanes 0 and 1     payload_values (behind C)     L of the next quad
//   black
//   ok          4       the border's polarity is the   gray_models: lane 0            the body (behind C)           L of the next quad
//                       family's
//   values      2048    the payload grid: value minus  the body (zeros, before C),    sharpen (behind D)            L of the next quad
//                       threshold, 0 where unknown     payload_values: a bit's lane
//   list        1024    the white and the negated      scores: a bit's lane           scores: lanes 0 and 1         L of the next quad
//                       black values, in bit order                                    (behind E)
//   sum         7484    + 4 of padding = 7488, what the build reports
//
// The three early `continue`s of the body, and why every lane of the wavefront takes them together: (1) slot 9 of the
// quad's record is 0 -- one global word, read by every lane; (2) ok is 0 -- one LDS word, read by every lane behind C;
// (3) no match or a negative margin -- the match comes out of a whole-wave reduction and the two scores are broadcast
// from lanes 0 and 1.  After each of them the next quad starts at L like after a full pass, and a quad's first write to
// the store (H) comes behind L: no lane still reads what the quad before left.
struct alignas(16) DecodeStore {  // the rows of smp, smpxy and bitxy start on 16 bytes: one 128-bit LDS access each
    double smp[DEC_BORDER_CAP][4];  // tagx, tagy, v, 1
    double values[DEC_GRID_CAP * DEC_GRID_CAP];
    double list[2][DEC_BITS_CAP];
    double smpxy[DEC_BORDER_CAP][2], bitxy[DEC_BITS_CAP][2];
    GrayModel white;
    double H[9];
    GrayModel black;
    int ok;
};
static_assert(sizeof(DecodeStore) == 7488, "k_decode: the plan and the LDS allocation disagree");

// Where a lane's border sample and its payload bit sit.  The steps ask a `Sites` instead of a table, so that k_decode_multi
// (below) can keep its families' sites in another form; the steps are templates over the store for the same reason.
// k_decode's Sites: the two tables of its store, the bit's cell from the family in the kernel's arguments.
struct DecodeSites {
    const DecodeStore &st;
    __device__ __forceinline__ void sample(int lane, double *tagx, double *tagy) const { *tagx = st.smpxy[lane][0]; *tagy = st.smpxy[lane][1]; }
    __device__ __forceinline__ void bit_cell(const FamilyDev &fam, int lane, int *bitx, int *bity) const { *bitx = fam.bit_x[lane]; *bity = fam.bit_y[lane]; }
    __device__ __forceinline__ void bit(int lane, double *tagx, double *tagy) const { *tagx = st.bitxy[lane][0]; *tagy = st.bitxy[lane][1]; }
};

// where a lane's payload bit sits: values[at], cell (x, y) of the grid
struct DecodeCell { int at, x, y; };
struct DecodeScores { float white_score, black_score, white_count, black_count; };
struct DecodeMatch { int id, hamming, rotation; };  // hamming 255: no code within maxhamming
struct UMin { __device__ __forceinline__ unsigned int operator()(unsigned int a, unsigned int b) const { return a < b ? a : b; } };

// ---- The steps of k_decode, in order.  Only decode_scores holds a barrier (E); the kernel body places the others.

// Tag-frame coordinates of the border samples and of the payload bits depend on the family only: computed once per
// workgroup (the pattern switch, two integer and four double divisions per lane), read from LDS for every quad.
// Writes smpxy, bitxy.
__device__ __forceinline__ void decode_tag_sites(DecodeStore &st, const FamilyDev &fam, int lane)
{
    const int wb = fam.width_at_border;
    if (lane < 8 * wb) {
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
        st.smpxy[lane][0] = 2 * (tagx01 - 0.5);
        st.smpxy[lane][1] = 2 * (tagy01 - 0.5);
    }
    if (lane < fam.nbits) {
        int bitx = fam.bit_x[lane], bity = fam.bit_y[lane];
        double tagx01 = (bitx + 0.5) / wb, tagy01 = (bity + 0.5) / wb;
        st.bitxy[lane][0] = 2 * (tagx01 - 0.5);
        st.bitxy[lane][1] = 2 * (tagy01 - 0.5);
    }
}

// Border samples, 8 patterns x width_at_border: a lane projects its sample and reads its pixel.  A sample outside the
// frame is left out of the sums upstream: here its row is all zeros, so that each of its terms is +0.0 and leaves a sum
// that started at +0.0 exactly as it is (no flag to read in decode_gray_models).  Reads H, smpxy; writes smp.
template <int CH, class Store, class Sites>
__device__ __forceinline__ void decode_border_samples(Store &st, const Sites &sites, const uint8_t *frame, const Geom &g, const FamilyDev &fam, int lane)
{
    if (lane < 8 * fam.width_at_border) {
        double tagx, tagy;
        sites.sample(lane, &tagx, &tagy);
        double px, py;
        hproject_dev(st.H, tagx, tagy, &px, &py);
        int ix = (int)px, iy = (int)py;
        const bool inside = !(ix < 0 || iy < 0 || ix >= g.w || iy >= g.h);
        const double gv = (double)gray_at<CH>(frame, g, inside ? ix : 0, inside ? iy : 0);
        st.smp[lane][0] = inside ? tagx : 0.0; st.smp[lane][1] = inside ? tagy : 0.0; st.smp[lane][2] = inside ? gv : 0.0; st.smp[lane][3] = inside ? 1.0 : 0.0;
    }
}

// Gray models of the white and the black border.  Upstream adds the samples one by one into 9 running sums per model;
// here lane a (0..8: white, 9..17: black) owns one sum and walks the samples in the same order, so every sum sees the
// same additions -- 4 x width_at_border steps of a wavefront instead of 8 x width_at_border x 9 of a single lane.  The
// sum's term is u*v with u, v picked from the sample's (x, y, gray, 1) row (x*1 and 1*1 are exact).  Both models are
// then solved at once: lane 0 solves white, lane 1 black (every lane runs the same code on its copy), and lane 0
// compares them at the tag's centre for the polarity.  Reads smp; writes white, black, ok.
template <class Store>
__device__ __forceinline__ void decode_gray_models(Store &st, const FamilyDev &fam, int lane)
{
    const int wb = fam.width_at_border, nsmp = 8 * wb;
    const int a = lane % 9, m = lane / 9;
    const int ku = a <= 2 ? 0 : (a <= 4 ? 1 : (a == 5 ? 3 : (a == 6 ? 0 : (a == 7 ? 1 : 2))));
    const int kv = a == 0 ? 0 : (a == 1 ? 1 : (a == 3 ? 1 : (a == 6 || a == 7 ? 2 : 3)));
    double acc = 0;
    if (lane < 18) {
        // patterns alternate white, black: a model's lanes visit only their own patterns (half the samples), in order
        for (int p0 = m * wb; p0 < nsmp; p0 += 2 * wb) {
            for (int smp = p0; smp < p0 + wb; smp++) {
                const double u = st.smp[smp][ku], v = st.smp[smp][kv];
                acc += u * v;
            }
        }
    }
    GrayModel gm;
    const int base = (lane & 1) * 9;
    gm.A[0] = __shfl(acc, base + 0); gm.A[1] = __shfl(acc, base + 1); gm.A[2] = __shfl(acc, base + 2);
    gm.A[3] = 0; gm.A[4] = __shfl(acc, base + 3); gm.A[5] = __shfl(acc, base + 4);
    gm.A[6] = 0; gm.A[7] = 0; gm.A[8] = __shfl(acc, base + 5);
    gm.B[0] = __shfl(acc, base + 6); gm.B[1] = __shfl(acc, base + 7); gm.B[2] = __shfl(acc, base + 8);
    gm.C[0] = 0; gm.C[1] = 0; gm.C[2] = 0;
    gm_solve_dev(gm);
    if (lane == 0) st.white = gm;
    if (lane == 1) st.black = gm;
    const double at0 = gm_interp_dev(gm, 0, 0);
    const double w0 = __shfl(at0, 0), b0 = __shfl(at0, 1);
    if (lane == 0) {
        bool flip = (w0 - b0 < 0);
        st.ok = (flip == (fam.reversed_border != 0)) ? 1 : 0;
    }
}

// Payload bits: a bit's lane projects its cell's centre, interpolates the gray value there and stores it minus the
// threshold between the two models; a cell whose four pixels are not all inside the frame keeps its 0.  Reads H, bitxy,
// white, black; writes values (one cell per lane).  Returns where the lane's bit sits.
template <int CH, class Store, class Sites>
__device__ __forceinline__ DecodeCell decode_payload_values(Store &st, const Sites &sites, const uint8_t *frame, const Geom &g, const FamilyDev &fam, int lane)
{
    const int wb = fam.width_at_border, tw = fam.total_width;
    int min_coord = (wb - tw) / 2;
    DecodeCell c = {0, 0, 0};
    if (lane < fam.nbits) {
        int bitx, bity;
        sites.bit_cell(fam, lane, &bitx, &bity);
        c.x = bitx - min_coord; c.y = bity - min_coord;
        c.at = tw * c.y + c.x;
        double tagx, tagy;
        sites.bit(lane, &tagx, &tagy);
        double px, py;
        hproject_dev(st.H, tagx, tagy, &px, &py);
        double v = value_for_pixel_dev<CH>(frame, g, px, py);
        if (v != -1) {
            double thresh = (gm_interp_dev(st.black, tagx, tagy) + gm_interp_dev(st.white, tagx, tagy)) / 2.0;
            st.values[c.at] = v - thresh;
        }
    }
    return c;
}

// Sharpening (upstream: the whole grid through a 3x3 Laplacian, then value + 0.25 * Laplacian): only the payload cells are
// read afterwards, so each bit's lane sharpens its own cell -- the same five terms in the same order.  No second grid,
// no pass over the 81 cells (two rounds with an integer division each), two barriers fewer.  Reads values.
template <class Store>
__device__ __forceinline__ double decode_sharpen(const Store &st, const FamilyDev &fam, const DecodeCell &c, int lane)
{
    const int tw = fam.total_width;
    double sharp_v = 0.0;
    if (lane < fam.nbits) {
        double sv = 0;
        if (c.y - 1 >= 0) sv += st.values[c.at - tw] * -1.0;
        if (c.x - 1 >= 0) sv += st.values[c.at - 1] * -1.0;
        sv += st.values[c.at] * 4.0;
        if (c.x + 1 <= tw - 1) sv += st.values[c.at + 1] * -1.0;
        if (c.y + 1 <= tw - 1) sv += st.values[c.at + tw] * -1.0;
        sharp_v = st.values[c.at] + 0.25 * sv;
    }
    return sharp_v;
}

// Code word and the two scores of the decision margin.  Upstream walks the bits in order and adds each value to the white
// or the black score (a float that takes a double: rounded after every addition).  The two scores are independent
// chains, so lane 0 adds the white values in bit order and lane 1 the negated black ones, from two compacted lists --
// ~20 steps of one add instead of 41 steps of compare, two conversions, add and select by every lane.  The code word is
// the ballot of "white".  Writes list, barrier E, reads list.
template <class Store>
__device__ __forceinline__ DecodeScores decode_scores(Store &st, const FamilyDev &fam, double sharp_v, int lane, unsigned long long *rcode)
{
    const bool isbit = lane < fam.nbits;
    const double v = isbit ? sharp_v : 0.0;
    const bool isw = isbit && v > 0;
    const unsigned long long wm = __ballot(isw), bm = __ballot(isbit && !isw);
    *rcode = __brevll(wm) >> (64 - fam.nbits);  // bit 0 of the family is the most significant bit of the code
    const unsigned long long below = (1ull << lane) - 1ull;
    if (isbit) st.list[isw ? 0 : 1][isw ? __popcll(wm & below) : __popcll(bm & below)] = isw ? v : -v;
    __syncthreads();  // E
    float score = 0;
    if (lane < 2) {
        const int cnt = lane == 0 ? __popcll(wm) : __popcll(bm);
        const double *list = st.list[lane];
        for (int k = 0; k < cnt; k++) score = (float)((double)score + list[k]);
    }
    DecodeScores s;
    s.white_score = __shfl(score, 0);
    s.black_score = __shfl(score, 1);
    s.white_count = (float)(1 + __popcll(wm));
    s.black_count = (float)(1 + __popcll(bm));
    return s;
}

// Code book.  Both searches return the first rotation whose best match is within maxhamming, there the lowest distance,
// then the lowest id: candidates are packed so that this order is the order of unsigned integers, and the wavefront
// takes their minimum.
// With the index (asl_common.h): lane (rotation, chunk) looks its bucket up, packed = rotation << 24 | distance << 16 | id.
__device__ __forceinline__ DecodeMatch decode_lookup_index(const FamilyDev &fam, unsigned long long rcode, int maxhamming, int lane)
{
    DecodeMatch m = {-1, 255, 0};
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
    best = wave_scan<true>(best, 0xFFFFFFFFu, UMin());
    if (best != 0xFFFFFFFFu) { m.id = (int)(best & 0xFFFFu); m.hamming = (int)((best >> 16) & 0xFFu); m.rotation = (int)(best >> 24); }
    return m;
}

// Without an index (a family wider than 48 bits): rotation by rotation against the whole book, packed = distance << 16 | id.
__device__ __forceinline__ DecodeMatch decode_lookup_book(const FamilyDev &fam, unsigned long long rcode, int maxhamming, int lane)
{
    DecodeMatch m = {-1, 255, 0};
#pragma unroll 1
    for (int ridx = 0; ridx < 4; ridx++) {
        unsigned int best = 0xFFFFFFFFu;
        for (int i = lane; i < fam.ncodes; i += 64) {
            const unsigned int dd = (unsigned int)__popcll(rcode ^ fam.codes[i]);
            best = UMin()(best, (dd << 16) | (unsigned int)i);
        }
        best = wave_scan<true>(best, 0xFFFFFFFFu, UMin());
        if ((best >> 16) <= (unsigned int)maxhamming) { m.id = (int)(best & 0xFFFFu); m.hamming = (int)(best >> 16); m.rotation = ridx; break; }
        rcode = rotate90_dev(rcode, fam.nbits);
    }
    return m;
}

// The detection record: lane 0 takes a slot, turns H by the match's rotation and projects the centre and the corners.
// Reads H.
template <class Store>
__device__ __forceinline__ void decode_emit(const Store &st, const DecodeMatch &m, float margin, int fr, unsigned long long qkey, DetRec *dets,
                                            unsigned int max_dets, long long *wcounters, int lane)
{
    if (lane == 0) {
        unsigned int di = (unsigned int)atomicAdd((unsigned long long *)&wcounters[CNT_NDETS], 1ull);
        if (di >= max_dets) { atomicAdd((unsigned long long *)&wcounters[CNT_OVERFLOW_DETS], 1ull); }
        else {
            const double C[4] = {1, 0, -1, 0}, Sn[4] = {0, 1, 0, -1};
            double c = C[m.rotation], s = Sn[m.rotation], Hr[9];
            for (int r = 0; r < 3; r++) {
                Hr[3 * r + 0] = st.H[3 * r + 0] * c + st.H[3 * r + 1] * s;
                Hr[3 * r + 1] = st.H[3 * r + 0] * -s + st.H[3 * r + 1] * c;
                Hr[3 * r + 2] = st.H[3 * r + 2];
            }
            DetRec *d = &dets[di];
            d->id = m.id; d->hamming = m.hamming; d->margin = margin; d->frame = fr; d->key = qkey;
            d->pose_ok = 0; d->pad = 0;
            hproject_dev(Hr, 0, 0, &d->center[0], &d->center[1]);
            for (int i = 0; i < 4; i++) {
                int tcx = (i == 1 || i == 2) ? 1 : -1, tcy = (i < 2) ? 1 : -1;
                hproject_dev(Hr, tcx, tcy, &d->corners[i][0], &d->corners[i][1]);
            }
        }
    }
}

// 5 waves per SIMD beats the 4 the allocator picks on its own; 6 spills too much.  At 5 the build reports
// 94 VGPRs for both instantiations and no scratch.
template <int CH>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) k_decode(const QuadRec *__restrict__ quads, const double *__restrict__ Hin,
                                               const long long *__restrict__ counters, unsigned int max_clusters,
                                               const uint8_t *__restrict__ frames, Geom g, FamilyDev fam, int maxhamming, DetRec *dets,
                                               unsigned int max_dets, long long *wcounters, const unsigned int *__restrict__ quad_list)
{
    __shared__ DecodeStore st;
    const int lane = threadIdx.x;
    PHASE_DECL();
    const unsigned int nq = tail_quad_count(counters, max_clusters);

    decode_tag_sites(st, fam, lane);
    const DecodeSites sites{st};
    for (unsigned int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();  // L
        PHASE_INIT();
        const unsigned int ci = quad_list[qi];
        if (Hin[10 * (size_t)ci + 9] == 0.0) continue;  // (1) no quad, wrong polarity, or singular homography
        const unsigned long long qkey = quads[ci].key;
        const int fr = (int)(qkey >> 48);
        const uint8_t *frame = frames + (size_t)fr * g.frame_pitch;
        if (lane < 9) st.H[lane] = Hin[10 * (size_t)ci + lane];
        __syncthreads();  // A
        PHASE(18);
        decode_border_samples<CH>(st, sites, frame, g, fam, lane);
        __syncthreads();  // B
        decode_gray_models(st, fam, lane);
        for (int i = lane; i < fam.total_width * fam.total_width; i += 64) st.values[i] = 0;
        __syncthreads();  // C
        if (!st.ok) continue;  // (2) the border's polarity is not the family's
        PHASE(19);
        const DecodeCell cell = decode_payload_values<CH>(st, sites, frame, g, fam, lane);
        __syncthreads();  // D
        const double sharp_v = decode_sharpen(st, fam, cell, lane);
        PHASE(20);
        unsigned long long rcode;
        const DecodeScores sc = decode_scores(st, fam, sharp_v, lane, &rcode);
        const DecodeMatch m = fam.idx_nch > 0 ? decode_lookup_index(fam, rcode, maxhamming, lane) : decode_lookup_book(fam, rcode, maxhamming, lane);
        PHASE(21);
        const float margin = fminf(sc.white_score / sc.white_count, sc.black_score / sc.black_count);
        if (!(margin >= 0) || m.hamming >= 255) continue;  // (3) no detection
        decode_emit(st, m, margin, fr, qkey, dets, max_dets, wcounters, lane);
        PHASE(23);
    }
    PHASE_FLUSH(16);
}

// ---- Several families in one detector: k_decode_multi, launched in place of k_decode when the detector holds more than
// one family.  One wavefront per quad, the steps above, the families of the table (FamilyTabDev, device memory) in a loop
// inside the quad: a quad is decoded against every family of its polarity and every family that accepts it yields a
// detection of its own, with id = id_base + local id (upstream's loop over its family list; no arbitration between
// families).  H is loaded once per quad; the border samples and the two gray models are taken once per border width --
// they depend on the family through width_at_border alone, and every candidate has the quad's polarity, so `ok` is a
// property of (quad, width) as well -- and the families of that width, next to each other in the table's `order`, read them.
//
// Storage plan: DecodeStore's per-quad members unchanged (same writers, readers and barriers); the tag sites in another
// form, because two 1 KB tables of doubles per family would be 8 KB for four.  Every site coordinate is
// 2 * ((n + 0.5) / width_at_border - 0.5) for an integer cell n along one axis: -1 .. width_at_border for the border
// patterns, the bit's cell for the payload, in all -8 .. 15 under asl_family_check's limits (total_width <= 16,
// width_at_border >= 2).  So a family keeps that one axis as doubles, computed by the expression decode_tag_sites uses
// (the same bits), and two cells per lane as bytes.
//
//   member      bytes   holds                              written by                    read by                      free after
//   axis        768     per family: the coordinate of      multi_tag_sites, once per     MultiSites (border_samples,  never
//                       cell n at [n + 8]                   workgroup, ahead of the       payload_values)
//   smpn        512     per family: the cells (x, y) of    first L
//                       lane's border sample
//   bitn        512     per family: the cells of lane's
//                       payload bit
//   H, smp, white, black, ok, values, list: 5436, as in DecodeStore, "next quad" reading "next width" for smp, white,
//                       black and ok, and "next family" for values and list
//   sum         7228    + 4 of padding = 7232, what the build reports: as many workgroups on a CU as k_decode's 7488
//
// Barriers: L, A per quad; B (border samples) and the gray models per width; C, D, E per family.  C also separates a
// family's zeroing of `values` from the cells the lanes then write; the zeroing itself comes behind E of the family
// before, whose last read of `values` (sharpen) is ahead of that E.  `list` of the family before is read behind its E
// by lanes 0 and 1, which reach this family's C and D only afterwards; this family writes it behind D.  A new width
// writes smp behind C of the family before (its readers, the model lanes, are ahead of that C), and white, black and
// ok behind B, which every lane reaches after its read of ok and of the models (payload_values, ahead of D).
//
// Early exits, all taken by the whole wavefront: (1) as in k_decode; inside the family loop a `continue` goes on to the
// next family, where every path meets barrier C (or B then C) again, so the test must be uniform: (4) the family's
// polarity against the quad's -- a word of the table and a word of the quad's record, each read by every lane from
// global memory that nothing writes during the kernel; (2) ok, one LDS word behind C; (3) the reduction and the two
// broadcasts, as in k_decode.  The loop's bounds and `order` are table words.  The width test that decides between
// B-then-C and C alone compares a table word with a value every lane derived from table words.
#define DEC_AXIS_LO 8   /* axis[f][n + DEC_AXIS_LO], n = -8 .. 15 */
#define DEC_AXIS_N 24
struct alignas(16) MultiStore {
    double smp[DEC_BORDER_CAP][4];
    double values[DEC_GRID_CAP * DEC_GRID_CAP];
    double list[2][DEC_BITS_CAP];
    double axis[FAM_MAX][DEC_AXIS_N];
    GrayModel white;
    double H[9];
    GrayModel black;
    signed char smpn[FAM_MAX][DEC_BORDER_CAP][2], bitn[FAM_MAX][DEC_BITS_CAP][2];
    int ok;
};
static_assert(sizeof(MultiStore) == 7232, "k_decode_multi: the plan and the LDS allocation disagree");
static_assert(DEC_GRID_CAP - 1 < DEC_AXIS_N - DEC_AXIS_LO && (DEC_GRID_CAP - 2) / 2 <= DEC_AXIS_LO, "k_decode_multi: a cell asl_family_check admits is off the axis");

struct MultiSites {
    const MultiStore &st;
    int f;
    __device__ __forceinline__ void sample(int lane, double *tagx, double *tagy) const
    {
        *tagx = st.axis[f][st.smpn[f][lane][0] + DEC_AXIS_LO]; *tagy = st.axis[f][st.smpn[f][lane][1] + DEC_AXIS_LO];
    }
    __device__ __forceinline__ void bit_cell(const FamilyDev &, int lane, int *bitx, int *bity) const { *bitx = st.bitn[f][lane][0]; *bity = st.bitn[f][lane][1]; }
    __device__ __forceinline__ void bit(int lane, double *tagx, double *tagy) const
    {
        *tagx = st.axis[f][st.bitn[f][lane][0] + DEC_AXIS_LO]; *tagy = st.axis[f][st.bitn[f][lane][1] + DEC_AXIS_LO];
    }
};

// decode_tag_sites for every family of the table.  Writes axis, smpn, bitn.
__device__ __forceinline__ void decode_multi_tag_sites(MultiStore &st, const FamilyTabDev *tab, int nf, int lane)
{
    for (int f = 0; f < nf; f++) {
        const int wb = tab->fam[f].width_at_border, nbits = tab->fam[f].nbits;
        if (lane < DEC_AXIS_N) {
            double tag01 = ((lane - DEC_AXIS_LO) + 0.5) / wb;
            st.axis[f][lane] = 2 * (tag01 - 0.5);
        }
        if (lane < 8 * wb) {
            const int pi = lane / wb, i = lane % wb;
            const int across = (pi & 3) == 0 ? -1 : ((pi & 3) == 1 ? 0 : ((pi & 3) == 2 ? wb : wb - 1));  // the pattern's line
            st.smpn[f][lane][0] = (signed char)(pi < 4 ? across : i);
            st.smpn[f][lane][1] = (signed char)(pi < 4 ? i : across);
        }
        if (lane < nbits) {
            st.bitn[f][lane][0] = (signed char)tab->fam[f].bit_x[lane];
            st.bitn[f][lane][1] = (signed char)tab->fam[f].bit_y[lane];
        }
    }
}

template <int CH>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) k_decode_multi(const QuadRec *__restrict__ quads, const double *__restrict__ Hin,
                                               const long long *__restrict__ counters, unsigned int max_clusters,
                                               const uint8_t *__restrict__ frames, Geom g, const FamilyTabDev *__restrict__ tab, int maxhamming,
                                               DetRec *dets, unsigned int max_dets, long long *wcounters, const unsigned int *__restrict__ quad_list)
{
    __shared__ MultiStore st;
    const int lane = threadIdx.x;
    const unsigned int nq = tail_quad_count(counters, max_clusters);
    const int nf = min(tab->n, FAM_MAX);

    decode_multi_tag_sites(st, tab, nf, lane);
    for (unsigned int qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();  // L
        const unsigned int ci = quad_list[qi];
        if (Hin[10 * (size_t)ci + 9] == 0.0) continue;  // (1) no quad, a polarity no family has, or singular homography
        const unsigned long long qkey = quads[ci].key;
        const int q_reversed = quads[ci].reversed_border;
        const int fr = (int)(qkey >> 48);
        const uint8_t *frame = frames + (size_t)fr * g.frame_pitch;
        if (lane < 9) st.H[lane] = Hin[10 * (size_t)ci + lane];
        __syncthreads();  // A
        int models_wb = 0;  // the border width the gray models in the store were fitted at
#pragma unroll 1
        for (int k = 0; k < nf; k++) {
            const int f = tab->order[k] & (FAM_MAX - 1);
            const FamilyDev &fam = tab->fam[f];
            if (fam.reversed_border != q_reversed) continue;  // (4) not a candidate for this quad
            const MultiSites sites{st, f};
            if (fam.width_at_border != models_wb) {
                models_wb = fam.width_at_border;
                decode_border_samples<CH>(st, sites, frame, g, fam, lane);
                __syncthreads();  // B
                decode_gray_models(st, fam, lane);
            }
            for (int i = lane; i < fam.total_width * fam.total_width; i += 64) st.values[i] = 0;
            __syncthreads();  // C
            if (!st.ok) continue;  // (2) the border's polarity at this width is not the quad's
            const DecodeCell cell = decode_payload_values<CH>(st, sites, frame, g, fam, lane);
            __syncthreads();  // D
            const double sharp_v = decode_sharpen(st, fam, cell, lane);
            unsigned long long rcode;
            const DecodeScores sc = decode_scores(st, fam, sharp_v, lane, &rcode);
            DecodeMatch m = fam.idx_nch > 0 ? decode_lookup_index(fam, rcode, maxhamming, lane) : decode_lookup_book(fam, rcode, maxhamming, lane);
            const float margin = fminf(sc.white_score / sc.white_count, sc.black_score / sc.black_count);
            if (!(margin >= 0) || m.hamming >= 255) continue;  // (3) no detection in this family
            m.id += tab->id_base[f];
            decode_emit(st, m, margin, fr, qkey, dets, max_dets, wcounters, lane);
        }
    }
}
