// S2-S4 on bit masks: adaptive threshold, connected components and gradient clusters.
//
// The ternary threshold image is never stored as bytes.  A row of 64 decimated pixels is two 64-bit masks
// (white, black; neither = "no contrast"), and the unit of work is the RUN -- a maximal stretch of one colour
// inside one 64-pixel word -- not the pixel: a 720p frame has ~230 k pixels, ~7 k runs and ~19 k boundary points.
//   k_seg_tile    one wavefront per 64x32 pixel tile: threshold by ballot (lane = column), then lane = (colour, row):
//                 run starts, the links to the row above and the union-find over run starts are mask algebra and
//                 per-run loops in LDS.  Writes the masks, parent[run start] = tile-local root, the local sizes at
//                 the local roots and one root mask per row.
//   k_tile_cut    3x3 dilation of the 4x4-tile extrema and the cut, one byte per tile
//   k_seg_border  the links that cross a tile edge (word seams in every row, row seams every 32 rows), one launch:
//                 global atomics, at most three joins per lane
//   k_seg_roots   tile-local roots -> global roots, sizes summed
//   k_seg_points  one wavefront per 64x63 pixel tile, lane = row, four tiles per workgroup: labels of the runs are
//                 fetched once per run into LDS, runs of small components are deleted from the masks, the four
//                 boundary-site masks are shifts and ANDs, and only pixels that emit a point are visited.  Its body is a
//                 sequence of named steps (segp_*); what lives where in its LDS, and until which barrier, is the plan
//                 table beside SegpStore; its packed words are stated once above that table, the rule for handing
//                 tiles to the dense launch once above the kernel.
// White is 8-connected, black 4-connected; only pixels with 1 <= x <= sw-2 initiate unions (upstream's row loops), so
// pixel sw-1 never joins its left neighbour: all of that is in the join mask J of a word.
// Mask layout: [frame][word column][row] (rows of one word column are contiguous: a wavefront's 32 / 64 rows are
// one coalesced access).

#define SEG_TH 32           /* rows of a k_seg_tile tile */
#define SEG_PH 63           /* rows a k_seg_points tile emits (it stages one more) */

// bits x of word x0/64 whose pixel may join its left neighbour / initiate links: 1 <= x0 + x <= sw - 2
__device__ __forceinline__ unsigned long long seg_join_mask(int x0, int sw)
{
    unsigned long long m = ~0ull;
    if (x0 == 0) m &= ~1ull;
    const int last = sw - 2 - x0;
    if (last < 0) return 0ull;
    if (last < 63) m &= (2ull << last) - 1ull;
    return m;
}

// pixels of the word that exist: x0 + x < sw
__device__ __forceinline__ unsigned long long seg_exist_mask(int x0, int sw)
{
    const int n = sw - x0;
    return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

// run starts of one colour: a set pixel starts a run unless its left neighbour is set and it may join it
__device__ __forceinline__ unsigned long long seg_starts(unsigned long long M, unsigned long long J) { return M & ~((M << 1) & J); }

// start bit of the run that holds bit x (S = starts of both colours or of x's colour; bit x must belong to a run)
__device__ __forceinline__ int seg_start_of(unsigned long long S, int x)
{
    return 63 - __clzll((long long)(S & (~0ull >> (63 - x))));
}

// length of the run that starts at bit sx of colour mask M
__device__ __forceinline__ int seg_run_len(unsigned long long M, unsigned long long J, int sx)
{
    const unsigned long long cont = (M >> 1) & (J >> 1);  // bit x: pixel x+1 continues the run of pixel x
    return 1 + __ffsll((long long)~(cont >> sx)) - 1;     // bit 63 of cont is clear, so ~(..) is never 0
}

// v_writelane_b32: put a wave-uniform value into one lane of a register (the builtin exists in the device pass only)
__device__ __forceinline__ unsigned int seg_writelane(unsigned int old, unsigned int val, int lane)
{
#if __HIP_DEVICE_COMPILE__
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "i"(lane));
    return old;
#else
    (void)val; (void)lane;
    return old;
#endif
}

// a tile's LDS slice is touched by one wavefront only: LDS operations of a wave execute in order, so "all lanes' stores
// before any lane's loads" needs no s_barrier, only that the compiler keeps the order
__device__ __forceinline__ void seg_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Table entry of run start (row, column): row * 65 + column.  With the odd row stride the starts of a vertical tag edge
// (same column in consecutive rows = the lanes of one access) sit in different LDS banks; a root is decoded once per run
// (seg_lrow / seg_lcol), the find and union loops only chase indices.  (Round 2's stride 64 measured 57 % of the LDS
// cycles as bank conflicts; rotating the columns per access instead cost three instructions per access: 0.30 -> 0.33 ms.)
#define SEG_LW 65
#define SEG_LN (SEG_TH * SEG_LW)
__device__ __forceinline__ unsigned int seg_lrow(unsigned int i) { return (i * 2017u) >> 17; }  // i / 65 for i < 2400

__device__ __forceinline__ unsigned int seg_lds_load(const unsigned int *L, unsigned int a)
{
    return __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & 0xFFFFu;
}

// roots of two entries, the two chains advancing together: one LDS round trip per step for both
__device__ __forceinline__ void seg_lds_find2(const unsigned int *L, unsigned int &a, unsigned int &b)
{
    unsigned int pa = seg_lds_load(L, a), pb = seg_lds_load(L, b);
    int guard = 0;
    while ((pa != a || pb != b) && guard++ < 4096) {
        a = pa; b = pb;
        pa = seg_lds_load(L, a); pb = seg_lds_load(L, b);
    }
}

// returns false if the guard ran out (never seen; reported loudly by the caller)
__device__ __forceinline__ bool seg_lds_union(unsigned int *L, unsigned int a, unsigned int b)
{
    for (int guard = 0; guard < 4096; guard++) {
        seg_lds_find2(L, a, b);
        if (a == b) return true;
        if (a < b) { unsigned int t = a; a = b; b = t; }
        unsigned int old = atomicMin(&L[a], b);  // entries hold only the parent index while unions run
        if (old == a) return true;
        a = old;
    }
    return false;
}

// Second half of the adaptive threshold's tile statistics: 3x3 dilation of the 4x4-tile extrema and the cut itself, one
// byte per tile: cut = min + (max - min) / 2, or 255 for a tile without contrast (max - min < 5; a real cut never
// exceeds 252).  A pixel is white iff gray > cut, black iff cut != 255 and not white.
// One thread per 4 x 4 block of tiles: per row of the block's neighbourhood (six rows, clamped into the image: a clamped row
// repeats a row of the neighbourhood, harmless for min / max) one 8-byte load per array (possibly unaligned: allowed for
// global loads) brings the six bytes t0-1 .. t0+4; the horizontal 3-min / 3-max of a row is computed once and shared by the
// up to three cuts above and below it.  12 loads for sixteen cuts (72 each done naively), and a sixteenth of the threads:
// with one thread per four tiles the kernel's 15 K workgroups took as long with 6 loads per thread as with 18 -- what it
// costs is getting the workgroups started.  At the row's ends the neighbour outside repeats the edge tile: a block at
// column 0 loads from its own first byte, a block that ends the row overwrites the byte beyond it (the buffers carry 8
// bytes of padding for the very last load).  The last block of a row, when tw is not a multiple of 4, goes byte by byte.
__global__ void __launch_bounds__(256) k_tile_cut(const uint8_t *__restrict__ tmin, const uint8_t *__restrict__ tmax, Geom g,
                                                  uint8_t *__restrict__ tcut)
{
    const int tw = g.tw, th = g.th, gx = (tw + 3) >> 2, gy = (th + 3) >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (i >= gx * gy) return;
    const int by = i / gx, t0 = (i - by * gx) * 4, y0 = by * 4;
    const uint8_t *pmin = tmin + (size_t)fr * tw * th, *pmax = tmax + (size_t)fr * tw * th;
    uint8_t *out = tcut + (size_t)fr * tw * th + t0;
    if (t0 + 4 <= tw) {
        const bool first = t0 == 0, last = t0 + 4 >= tw;
        unsigned int hmn[6], hmx[6];  // per neighbourhood row y0-1 .. y0+4: the horizontal 3-min / 3-max of the four tiles, a byte each
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const unsigned int row = (unsigned int)min(max(y0 - 1 + r, 0), th - 1) * (unsigned int)tw;
            unsigned long long a, b;
            __builtin_memcpy(&a, pmin + row + t0 - (first ? 0 : 1), 8);
            __builtin_memcpy(&b, pmax + row + t0 - (first ? 0 : 1), 8);
            if (first) { a = (a << 8) | (a & 255ull); b = (b << 8) | (b & 255ull); }
            if (last) { a = (a & ~(255ull << 40)) | (((a >> 32) & 255ull) << 40); b = (b & ~(255ull << 40)) | (((b >> 32) & 255ull) << 40); }
            unsigned int pn = 0, px = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned int n0 = (unsigned int)(a >> (8 * k)) & 255u, n1 = (unsigned int)(a >> (8 * k + 8)) & 255u, n2 = (unsigned int)(a >> (8 * k + 16)) & 255u;
                const unsigned int x0 = (unsigned int)(b >> (8 * k)) & 255u, x1 = (unsigned int)(b >> (8 * k + 8)) & 255u, x2 = (unsigned int)(b >> (8 * k + 16)) & 255u;
                pn |= min(min(n0, n1), n2) << (8 * k);
                px |= max(max(x0, x1), x2) << (8 * k);
            }
            hmn[r] = pn; hmx[r] = px;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (y0 + r >= th) break;
            unsigned int packed = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const unsigned int mn = min(min((hmn[r] >> (8 * k)) & 255u, (hmn[r + 1] >> (8 * k)) & 255u), (hmn[r + 2] >> (8 * k)) & 255u);
                const unsigned int mx = max(max((hmx[r] >> (8 * k)) & 255u, (hmx[r + 1] >> (8 * k)) & 255u), (hmx[r + 2] >> (8 * k)) & 255u);
                packed |= (mx - mn < (unsigned int)MIN_WHITE_BLACK_DIFF ? 255u : mn + (mx - mn) / 2u) << (8 * k);
            }
            __builtin_memcpy(out + (size_t)(y0 + r) * tw, &packed, 4);
        }
        return;
    }
    for (int ty = y0; ty < min(y0 + 4, th); ty++)
        for (int tx = t0; tx < tw; tx++) {
            int mn = 255, mx = 0;
            for (int dy = -1; dy <= 1; dy++) {
                const int yy = min(max(ty + dy, 0), th - 1);
                for (int dx = -1; dx <= 1; dx++) {
                    const int xx = min(max(tx + dx, 0), tw - 1);
                    mn = min(mn, (int)pmin[yy * tw + xx]);
                    mx = max(mx, (int)pmax[yy * tw + xx]);
                }
            }
            out[(size_t)ty * tw + tx - t0] = (uint8_t)(mx - mn < MIN_WHITE_BLACK_DIFF ? 255 : mn + (mx - mn) / 2);
        }
}

#ifndef SEG_TILE_WAVES
#define SEG_TILE_WAVES 4  /* tiles (wavefronts) of a k_seg_tile workgroup: 123 K one-wave workgroups per batch cost 0.087 ms on frames without contrast, four tiles per workgroup 0.073 */
#endif
#define SEG_CAP 512  /* runs (and links) of a tile the common launch labels; a tile with more goes on the dense list (k_seg_tile_dense) */

// bits 0 .. x of a word
__device__ __forceinline__ unsigned long long seg_upto(int x) { return ~0ull >> (63 - x); }

// ---- threshold of one 64 x 32 tile.  Lane = (row r' of a 16-row half, 16-pixel segment s): the 4 + 4 cuts of the lane's
// tile columns and the gray tile as two 16-byte loads per lane, all in flight together (addresses clamped into the image,
// results masked).  A tile without contrast (every cut 255) is known from the cuts alone and skips the compares.
// Otherwise the byte compares give 16 white + 16 black bits per lane and half; the four segments of a row sit in one quad
// (DPP broadcasts assemble the 64-bit row masks), and two ds_bpermute per half move them to lane = (colour, row).
// Returns the mask of lane = (colour lane >> 5, row lane & 31).
__device__ __forceinline__ unsigned long long seg_threshold_tile(const uint8_t *__restrict__ dg, const uint8_t *__restrict__ tc, const Geom &g, int x0, int y0, int lane)
{
    const int sw = g.sw, sh = g.sh;
    const int seg = lane & 3, rq = lane >> 2;
    const int xs = x0 + 16 * seg;
    const bool whole = xs + 16 <= sw;  // the segment lies inside the row: one 16-byte load
    uint4 px[2];
    unsigned int cut[2][4];
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const unsigned int yy = (unsigned int)min(y0 + 16 * hf + rq, sh - 1);
        const unsigned int trow = (unsigned int)min((int)yy / TILESZ, g.th - 1) * (unsigned int)g.tw;
#pragma unroll
        for (int q = 0; q < 4; q++) cut[hf][q] = tc[trow + (unsigned int)min((xs >> 2) + q, g.tw - 1)];
    }
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const unsigned int yy = (unsigned int)min(y0 + 16 * hf + rq, sh - 1);
        const uint8_t *row = dg + (size_t)yy * (unsigned int)sw;
        if (whole) {
            px[hf] = *reinterpret_cast<const uint4 *>(row + xs);  // unaligned when sw is not a multiple of 16: allowed for global loads
        } else {
            unsigned int d[4] = {0, 0, 0, 0};
            for (int k = 0; k < 16; k++) d[k >> 2] |= (unsigned int)row[min(xs + k, sw - 1)] << (8 * (k & 3));
            px[hf] = make_uint4(d[0], d[1], d[2], d[3]);
        }
    }
    const unsigned int cmin = min(min(min(cut[0][0], cut[0][1]), min(cut[0][2], cut[0][3])), min(min(cut[1][0], cut[1][1]), min(cut[1][2], cut[1][3])));
    if (__ballot(cmin != 255u) == 0ull) return 0ull;
    unsigned int xlo[2], xhi[2];
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const unsigned int d[4] = {px[hf].x, px[hf].y, px[hf].z, px[hf].w};
        unsigned int wbits = 0, cbits = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned int c = cut[hf][q];
            if (c != 255u) cbits |= 0xFu << (4 * q);
#pragma unroll
            for (int k = 0; k < 4; k++) wbits |= (((d[q] >> (8 * k)) & 255u) > c ? 1u : 0u) << (4 * q + k);
        }
        const int left = sw - xs;  // pixels of the segment that exist
        cbits &= left >= 16 ? 0xFFFFu : (left <= 0 ? 0u : (1u << left) - 1u);
        wbits &= cbits;
        const unsigned int pk = wbits | ((cbits & ~wbits) << 16);  // white | black << 16
        const unsigned int q0 = quad_bcast<0>(pk), q1 = quad_bcast<1>(pk), q2 = quad_bcast<2>(pk), q3 = quad_bcast<3>(pk);
        const bool blk = (seg & 1) != 0;  // lane 4r' keeps the white mask of its row, lane 4r' + 1 the black one
        xlo[hf] = blk ? ((q0 >> 16) | (q1 & 0xFFFF0000u)) : ((q0 & 0xFFFFu) | (q1 << 16));
        xhi[hf] = blk ? ((q2 >> 16) | (q3 & 0xFFFF0000u)) : ((q2 & 0xFFFFu) | (q3 << 16));
    }
    // lane L = (colour L >> 5, row L & 31): row r lives in half r >> 4, quad r & 15
    const int src = 4 * (lane & 15) + (lane >> 5);
    const bool second = (lane & 16) != 0;
    const unsigned int lo0 = (unsigned int)__shfl((int)xlo[0], src), hi0 = (unsigned int)__shfl((int)xhi[0], src);
    const unsigned int lo1 = (unsigned int)__shfl((int)xlo[1], src), hi1 = (unsigned int)__shfl((int)xhi[1], src);
    return ((unsigned long long)(second ? hi1 : hi0) << 32) | (second ? lo1 : lo0);
}

// The links of a row's pixels to the row above, inside a tile (lane = (colour, row); Mp = the mask of the row above, 0 for
// the tile's first row).  Every pair of touching runs gets at least one union; a stretch of vertically adjacent pixels is
// one contact.  link[0] up, link[1] up-left, link[2] up-right; the diagonals are white's alone (isw).
__device__ __forceinline__ void seg_links(unsigned long long M, unsigned long long Mp, unsigned long long J, bool isw, unsigned long long (&link)[3])
{
    const unsigned long long U = M & Mp & J;
    link[0] = U & ~(U << 1);
    link[1] = isw ? (M & J & (Mp << 1) & ~Mp) : 0ull;               // up-left, only where "up" does not already connect
    link[2] = isw ? (M & J & (Mp >> 1) & ~(Mp & (J >> 1))) : 0ull;  // up-right, unless up connects and x+1 joins x above
}

// Run word of k_seg_tile's run list: row 5 | start column 6 | length - 1 (6 bits, the word's top field)
static_assert(SEG_TH <= 32, "run word: row");
__device__ __forceinline__ unsigned int seg_runw_pack(int row, int sx, int len) { return (unsigned int)row | ((unsigned int)sx << 5) | ((unsigned int)(len - 1) << 11); }
__device__ __forceinline__ unsigned int seg_runw_row(unsigned int e) { return e & 31u; }
__device__ __forceinline__ unsigned int seg_runw_col(unsigned int e) { return (e >> 5) & 63u; }
__device__ __forceinline__ unsigned int seg_runw_len(unsigned int e) { return (e >> 11) + 1u; }

// The common launch: threshold, masks out, and the components of the tile by union-find over RUN NUMBERS.  The runs of a
// tile are numbered in the order (colour, row, column) -- a prefix sum over the lanes' run counts -- so the tables are as
// long as the tile has runs (some eighty in a tile that a tag crosses), not 64 x 32 entries: 4.4 KB of LDS per wavefront,
// a CU holds its 32 wavefronts.  Within a colour the numbering is raster order, and all runs of a component have one
// colour: hanging the larger number under the smaller one keeps the smallest raster index as the root, the canonical label.
// The rows of a tile are very unequal (a tag's payload rows hold most of the runs, the rows beside a tag none), so a row's
// lane only LISTS its links and runs (short loops without a dependent memory access) and the unions / finds are done one
// item per lane, by all 64 lanes.  A tile with more than SEG_CAP runs or links (noise, fine stripes) goes on the dense list.
__global__ void __launch_bounds__(64 * SEG_TILE_WAVES) k_seg_tile(const uint8_t *__restrict__ dgray, const uint8_t *__restrict__ tcut, Geom g, int nwx, int ntiles,
                                                 unsigned long long *__restrict__ wmask, unsigned long long *__restrict__ bmask,
                                                 unsigned int *__restrict__ parent, unsigned int *__restrict__ sizes,
                                                 unsigned long long *__restrict__ rootmask, uint4 *__restrict__ edges, unsigned int *__restrict__ dense_list,
                                                 long long *counters)
{
    // every wavefront of the workgroup has its own tile and its own slice of the tables (nothing is shared: no barrier)
    __shared__ unsigned int Ls[SEG_TILE_WAVES][SEG_CAP];          // per run: low 16 bits parent, high 16 bits (roots) pixel count
    __shared__ unsigned int WLs[SEG_TILE_WAVES][SEG_CAP];         // links (a | b << 16), then the runs (run words: seg_runw_pack)
    __shared__ unsigned long long RMKs[SEG_TILE_WAVES][SEG_TH];   // per row: the run starts that are roots (both colours)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int *const L = Ls[wave], *const WL = WLs[wave];
    unsigned long long *const RMK = RMKs[wave];
    const int tile = blockIdx.x * SEG_TILE_WAVES + wave, fr = blockIdx.z;
    if (tile >= ntiles) return;
    const int wx = tile % nwx, x0 = wx * 64, y0 = (tile / nwx) * SEG_TH;
    const int sw = g.sw, sh = g.sh;
    PHASE_DECL();
    PHASE_INIT();
    unsigned long long M = 0;
    if (g.tw > 0 && g.th > 0)  // an image smaller than one 4x4 tile is "no contrast" everywhere
        M = seg_threshold_tile(dgray + (size_t)fr * g.npix, tcut + (size_t)fr * g.tw * g.th, g, x0, y0, lane);
    PHASE(2);
    const int r = lane & 31;
    const bool isw = lane < 32;
    const int y = y0 + r;
    if (y >= sh) M = 0;  // rows below the image were filled from its last row
    const size_t mi = ((size_t)fr * nwx + wx) * sh + y;
    if (y < sh) { if (isw) wmask[mi] = M; else bmask[mi] = M; }
    {
        // the tile's first and last pixel column, one bit per row and colour: all the seam pass needs to know whether a row
        // of a word seam can hold a link at all (it then reads 32 bytes per tile pair instead of 48 per row)
        const unsigned long long el = __ballot((M & 1ull) != 0ull), er = __ballot((M >> 63) != 0ull);
        if (lane == 0) edges[(size_t)fr * ntiles + tile] = make_uint4((unsigned int)el, (unsigned int)(el >> 32), (unsigned int)er, (unsigned int)(er >> 32));
    }
    PHASE(8);
    if (__ballot(M != 0) == 0ull) {  // no contrast anywhere in the tile: no runs, no roots
        if (isw && y < sh) rootmask[mi] = 0ull;
        PHASE_FLUSH(48);
        return;
    }
    // ---- lane = (colour, row): runs and their links to the row above (inside the tile)
    const unsigned long long J = seg_join_mask(x0, sw);
    const unsigned long long S = seg_starts(M, J);
    unsigned long long Mp = __shfl_up(M, 1), Sp = __shfl_up(S, 1);
    if (r == 0) { Mp = 0; Sp = 0; }  // the row above belongs to another tile: k_seg_border
    unsigned long long link[3];
    seg_links(M, Mp, J, isw, link);
    const unsigned int nlinks_lane = (unsigned int)(__popcll(link[0]) + __popcll(link[1]) + __popcll(link[2])), nruns_lane = (unsigned int)__popcll(S);
    // inclusive prefix sums; at most 64 x 96 links and 64 x 32 runs: both fit 16 bits
    const unsigned int incl = wave_scan<false>(nlinks_lane | (nruns_lane << 16), 0u, [](unsigned int a, unsigned int b) { return a + b; });
    const unsigned int tot = readlane(incl, 63);
    const int nlinks = (int)(tot & 0xFFFFu), nruns = (int)(tot >> 16);
    PHASE_COUNT(12, nlinks); PHASE_COUNT(13, nruns); PHASE_COUNT(14, 1);
    if (nlinks > SEG_CAP || nruns > SEG_CAP) {
        if (lane == 0) dense_list[atomicAdd((unsigned long long *)&counters[CNT_DENSE_SEG], 1ull)] = (unsigned int)fr * (unsigned int)ntiles + (unsigned int)tile;
        PHASE_FLUSH(48);
        return;
    }
    const unsigned int rb = (incl >> 16) - nruns_lane;          // number of this lane's first run
    const unsigned int rbp = (unsigned int)__shfl_up((int)rb, 1);  // ... of the first run of the row above (same colour)
    for (int i = lane; i < nruns; i += 64) L[i] = (unsigned int)i;
    if (lane < SEG_TH) RMK[lane] = 0ull;
    {
        unsigned int j = (incl & 0xFFFFu) - nlinks_lane;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            unsigned long long m = link[t];
            const int dx = t == 0 ? 0 : (t == 1 ? -1 : 1);
            while (m) {
                const int bx = __ffsll((long long)m) - 1;
                m &= m - 1;
                const unsigned int a = rb + (unsigned int)__popcll(S & seg_upto(bx)) - 1u;
                const unsigned int b = rbp + (unsigned int)__popcll(Sp & seg_upto(bx + dx)) - 1u;
                WL[j++] = a | (b << 16);
            }
        }
    }
    seg_wave_sync();
    PHASE(3);
    {
        bool bad = false;
        for (int i = lane; i < nlinks; i += 64) {
            const unsigned int e = WL[i];
            bad |= !seg_lds_union(L, e & 0xFFFFu, e >> 16);
        }
        if (bad) atomicAdd((unsigned long long *)&counters[CNT_UF_GUARD], 1ull);
    }
    seg_wave_sync();
    PHASE(9);
    // ---- the run list (its index is the run's number): where the run starts and how long it is
    {
        unsigned int j = rb;
        unsigned long long m = S;
        while (m) {
            const int sx = __ffsll((long long)m) - 1;
            m &= m - 1;
            WL[j++] = seg_runw_pack(r, sx, seg_run_len(M, J, sx));
        }
    }
    seg_wave_sync();
    // ---- every run: root, pixel count to the root, global parent entry (the unions are over: a run that is its own root
    // stays one); two runs per trip, their finds advancing together
    unsigned int *P = parent + (size_t)fr * g.npix;
    for (int i = lane; i < nruns; i += 128) {
        const bool two = i + 64 < nruns;
        const unsigned int i0 = (unsigned int)i, i1 = two ? i0 + 64u : i0;
        const unsigned int e0 = WL[i0], e1 = WL[i1];
        unsigned int r0 = i0, r1 = i1;
        seg_lds_find2(L, r0, r1);
        const unsigned int f0 = WL[r0], f1 = WL[r1];  // where the roots start
        atomicAdd(&L[r0], seg_runw_len(e0) << 16);
        if (two) atomicAdd(&L[r1], seg_runw_len(e1) << 16);
        // i is not a root: nobody adds to it, and finds passing through see an ancestor either way
        if (r0 != i0) L[i0] = r0; else atomicOr(&RMK[seg_runw_row(e0)], 1ull << seg_runw_col(e0));
        if (two) { if (r1 != i1) L[i1] = r1; else atomicOr(&RMK[seg_runw_row(e1)], 1ull << seg_runw_col(e1)); }
        auto pix = [&](unsigned int e) { return (unsigned int)((y0 + (int)seg_runw_row(e)) * sw + x0 + (int)seg_runw_col(e)); };  // frame index of a run word's start
        P[pix(e0)] = pix(f0);
        if (two) P[pix(e1)] = pix(f1);
    }
    seg_wave_sync();
    PHASE(10);
    // ---- roots: local size out, root mask of the row
    const unsigned long long rm = RMK[r];  // white and black roots of the row
    {
        unsigned int *SZ = sizes + (size_t)fr * g.npix;
        unsigned long long m = rm & S;     // this lane's colour
        while (m) {
            const int sx = __ffsll((long long)m) - 1;
            m &= m - 1;
            SZ[(size_t)y * sw + x0 + sx] = L[rb + (unsigned int)__popcll(S & seg_upto(sx)) - 1u] >> 16;
        }
    }
    if (isw && y < sh) rootmask[mi] = rm;
    PHASE(11);
    PHASE_FLUSH(48);
}

// The tiles the common launch put on the dense list (more runs or links than its tables hold: noise, one-pixel stripes):
// the same labelling over a table with one entry per pixel of the tile (entry of run start (row, column) = row * 65 +
// column: with the odd stride the starts of a vertical edge sit in different LDS banks), every lane walking the links and
// runs of its own row.  One wavefront per tile, grid-stride over the list; the masks are read back from memory.
__global__ void __launch_bounds__(64) k_seg_tile_dense(Geom g, int nwx, int ntiles, const unsigned long long *__restrict__ wmask,
                                                       const unsigned long long *__restrict__ bmask, unsigned int *__restrict__ parent,
                                                       unsigned int *__restrict__ sizes, unsigned long long *__restrict__ rootmask,
                                                       const unsigned int *__restrict__ dense_list, long long *counters)
{
    __shared__ __attribute__((aligned(16))) unsigned int L[SEG_LN];
    const int lane = threadIdx.x & 63, r = lane & 31;
    const bool isw = lane < 32;
    const int sw = g.sw, sh = g.sh;
    const long long n = counters[CNT_DENSE_SEG];
    for (long long w = blockIdx.x; w < n; w += gridDim.x) {
        const unsigned int id = dense_list[w];
        const int fr = (int)(id / (unsigned int)ntiles), tile = (int)(id % (unsigned int)ntiles);
        const int wx = tile % nwx, x0 = wx * 64, y0 = (tile / nwx) * SEG_TH;
        const int y = y0 + r;
        const size_t mi = ((size_t)fr * nwx + wx) * sh + y;
        const unsigned long long M = y < sh ? (isw ? wmask[mi] : bmask[mi]) : 0ull;
        const unsigned long long J = seg_join_mask(x0, sw);
        const unsigned long long S = seg_starts(M, J);
        unsigned long long Mp = __shfl_up(M, 1), Sp = __shfl_up(S, 1);
        if (r == 0) { Mp = 0; Sp = 0; }
        seg_wave_sync();  // the previous tile's last reads of the table are done
#pragma unroll
        for (int k = 0; k < (SEG_LN + 255) / 256; k++) {  // identity, 4 entries per lane and store
            const unsigned int i = (unsigned int)(k * 256 + 4 * lane);
            if (i < (unsigned int)SEG_LN) *reinterpret_cast<uint4 *>(&L[i]) = make_uint4(i, i + 1, i + 2, i + 3);
        }
        seg_wave_sync();
        const unsigned int rbase = (unsigned int)(r * SEG_LW);
        {
            unsigned long long link[3];
            seg_links(M, Mp, J, isw, link);
            bool bad = false;
#pragma unroll
            for (int t = 0; t < 3; t++) {
                unsigned long long m = link[t];
                const int dx = t == 0 ? 0 : (t == 1 ? -1 : 1);
                while (m) {
                    const int bx = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    bad |= !seg_lds_union(L, rbase + (unsigned int)seg_start_of(S, bx), rbase - (unsigned int)SEG_LW + (unsigned int)seg_start_of(Sp, bx + dx));
                }
            }
            if (bad) atomicAdd((unsigned long long *)&counters[CNT_UF_GUARD], 1ull);
        }
        seg_wave_sync();
        unsigned int *P = parent + (size_t)fr * g.npix;
        unsigned long long rm = 0;  // the runs of this lane that are roots (the unions are over: final)
        {
            unsigned long long m = S;
            while (m) {
                const int sx0 = __ffsll((long long)m) - 1;
                m &= m - 1;
                const bool two = m != 0ull;
                const int sx1 = two ? __ffsll((long long)m) - 1 : sx0;
                if (two) m &= m - 1;
                const unsigned int i0 = rbase + (unsigned int)sx0, i1 = rbase + (unsigned int)sx1;
                unsigned int r0 = i0, r1 = i1;
                seg_lds_find2(L, r0, r1);
                atomicAdd(&L[r0], (unsigned int)seg_run_len(M, J, sx0) << 16);
                if (two) atomicAdd(&L[r1], (unsigned int)seg_run_len(M, J, sx1) << 16);
                if (r0 != i0) L[i0] = r0; else rm |= 1ull << sx0;
                if (two) { if (r1 != i1) L[i1] = r1; else rm |= 1ull << sx1; }
                const unsigned int q0 = seg_lrow(r0), q1 = seg_lrow(r1);
                P[(size_t)y * sw + x0 + sx0] = (unsigned int)((y0 + (int)q0) * sw + x0 + (int)(r0 - q0 * SEG_LW));
                if (two) P[(size_t)y * sw + x0 + sx1] = (unsigned int)((y0 + (int)q1) * sw + x0 + (int)(r1 - q1 * SEG_LW));
            }
        }
        seg_wave_sync();
        {
            unsigned int *SZ = sizes + (size_t)fr * g.npix;
            unsigned long long m = rm;
            while (m) {
                const int sx = __ffsll((long long)m) - 1;
                m &= m - 1;
                SZ[(size_t)y * sw + x0 + sx] = L[rbase + (unsigned int)sx] >> 16;
            }
        }
        rm |= __shfl_down(rm, 32);  // white and black roots of the row
        if (isw && y < sh) rootmask[mi] = rm;
    }
}

// Links across tile edges go through global memory.  A join is a handful of dependent L2 round trips (two finds and an
// atomicMin), so the links are spread over as many lanes as possible: nobody executes more than three joins.
__device__ __forceinline__ bool seg_global_join(unsigned int *P, unsigned int a, unsigned int b)
{
    for (int guard = 0; guard < (1 << 16); guard++) {
        // both finds advance together: every step is one round trip to L2 for the two of them, not two
        unsigned int pa = __hip_atomic_load(&P[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned int pb = __hip_atomic_load(&P[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int hops = 0;
        while ((pa != a || pb != b) && hops++ < (1 << 22)) {
            a = pa; b = pb;
            pa = __hip_atomic_load(&P[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pb = __hip_atomic_load(&P[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (a == b) return true;
        if (a < b) { unsigned int t = a; a = b; b = t; }  // a > b: hang a under b
        unsigned int old = atomicMin(&P[a], b);
        if (old == a) return true;  // a was still a root: linked
        a = old;                    // somebody re-parented a meanwhile; (old, b) still has to be joined
    }
    return false;  // never seen; the caller reports it loudly
}

// The seam between a word and the word on its left, one lane per (word column >= 1, row): pixel x0 joins pixel x0-1 of
// its row, and inside a tile row block the two white diagonals that cross the seam.
__device__ __forceinline__ void seg_border_cols_body(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                     const uint4 *__restrict__ edges, int ntiles, const Geom &g, int nwx,
                                                     unsigned int *__restrict__ parent, long long *counters, unsigned int blk)
{
    const int sw = g.sw, sh = g.sh;
    const size_t per_frame = (size_t)nwx * sh, seams = (size_t)(nwx - 1) * sh;
    const size_t i0 = (size_t)blk * 64 + threadIdx.x;
    const bool inrange = i0 < seams * g.nframes;  // no lane leaves before the shuffles below: they read the neighbour's registers
    const size_t i = inrange ? i0 : 0;
    const int fr = (int)(i / seams);
    const int rem = (int)(i - (size_t)fr * seams);
    const int wx = 1 + rem / sh, y = rem % sh, x0 = wx * 64;
    const unsigned long long *wm = wmask + (size_t)fr * per_frame, *bm = bmask + (size_t)fr * per_frame;
    const size_t m0 = (size_t)wx * sh + y;
    // a row of the seam can hold a link only if a pixel sits on either side of it: known from the tiles' edge summaries
    // (k_seg_tile), the same 16 bytes for the 32 rows of a tile; the masks themselves are read by the rows that have one
    const size_t et = (size_t)fr * ntiles + (size_t)(y / SEG_TH) * nwx + wx;
    const uint4 ec = edges[et], el = edges[et - 1];
    const bool seam = inrange && ((((ec.x | ec.y) | (el.z | el.w)) >> (y % SEG_TH)) & 1u) != 0u;
    if (__ballot(seam) == 0ull) return;
    const bool diag = seam && y > 0 && (y % SEG_TH) != 0;  // rows y and y-1 in one tile row block (the row seams are k_seg_border_rows')
    const unsigned long long W = seam ? wm[m0] : 0ull, B = seam ? bm[m0] : 0ull, Wl = seam ? wm[m0 - sh] : 0ull, Bl = seam ? bm[m0 - sh] : 0ull;
    const unsigned long long Wp = diag ? wm[m0 - 1] : 0ull, Wlp = diag ? wm[m0 - sh - 1] : 0ull;
    unsigned int *P = parent + (size_t)fr * g.npix;
    const unsigned long long J = seam ? seg_join_mask(x0, sw) : 0ull, Jl = seam ? seg_join_mask(x0 - 64, sw) : 0ull;
    auto gidx = [&](int word, int yy, int bit) { return (unsigned int)(yy * sw + word * 64 + bit); };
    // up to four links per lane: same row white / black, and the two white diagonals across the seam
    unsigned int ja[4], jb[4];
    bool jv[4] = {false, false, false, false};
    if (J & 1ull) {
        if ((W & 1ull) && (Wl >> 63)) { jv[0] = true; ja[0] = gidx(wx, y, 0); jb[0] = gidx(wx - 1, y, seg_start_of(seg_starts(Wl, Jl), 63)); }
        if ((B & 1ull) && (Bl >> 63)) { jv[1] = true; ja[1] = gidx(wx, y, 0); jb[1] = gidx(wx - 1, y, seg_start_of(seg_starts(Bl, Jl), 63)); }
        if ((W & 1ull) && (Wlp >> 63)) { jv[2] = true; ja[2] = gidx(wx, y, 0); jb[2] = gidx(wx - 1, y - 1, seg_start_of(seg_starts(Wlp, Jl), 63)); }  // (x0, y) -> (x0-1, y-1)
    }
    if ((Jl >> 63) && (Wl >> 63) && (Wp & 1ull)) { jv[3] = true; ja[3] = gidx(wx - 1, y, seg_start_of(seg_starts(Wl, Jl), 63)); jb[3] = gidx(wx, y - 1, 0); }  // (x0-1, y) -> (x0, y-1)
    // first hop of all links together (a run start's parent is its tile-local root).  A seam that runs along a tag border
    // gives the same pair of roots in every row of the tile: the lane whose upper neighbour holds the same pair leaves the
    // link to it -- equal parents mean the runs are already connected to the neighbour's, so one join serves them all.
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (jv[t]) {
            ja[t] = __hip_atomic_load(&P[ja[t]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            jb[t] = __hip_atomic_load(&P[jb[t]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const unsigned long long key = jv[t] ? (((unsigned long long)ja[t] << 32) | jb[t]) : ~0ull;
        const unsigned long long up = __shfl_up(key, 1);
        // the neighbour must be the row above in the same word column of the same frame (y > 0): parents are frame-local
        // indices, an equal pair in another frame or column says nothing
        const bool dup = jv[t] && threadIdx.x > 0 && y > 0 && up == key;
        if (jv[t] && !dup) ok &= seg_global_join(P, ja[t], jb[t]);
    }
    if (!ok) atomicAdd((unsigned long long *)&counters[CNT_UF_GUARD], 1ull);
}

// The seam between two tile row blocks (rows 32k-1 and 32k), one lane per pixel of row 32k: the lane of the first pixel
// of a contact (or of a diagonal-only contact) joins the two runs.
__device__ __forceinline__ void seg_border_rows_body(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                     const Geom &g, int nwx, unsigned int *__restrict__ parent, long long *counters, int wx, int rb, int fr)
{
    const int sw = g.sw, sh = g.sh;
    const int y = (rb + 1) * SEG_TH, x0 = wx * 64;
    const int bx = threadIdx.x;
    const size_t per_frame = (size_t)nwx * sh;
    const unsigned long long *wm = wmask + (size_t)fr * per_frame, *bm = bmask + (size_t)fr * per_frame;
    const size_t m0 = (size_t)wx * sh + y;
    const unsigned long long W = wm[m0], B = bm[m0], Wp = wm[m0 - 1], Bp = bm[m0 - 1];
    if ((W | B) == 0ull || (Wp | Bp) == 0ull) return;
    unsigned int *P = parent + (size_t)fr * g.npix;
    const unsigned long long J = seg_join_mask(x0, sw);
    const unsigned long long bit = 1ull << bx;
    auto gidx = [&](int word, int yy, int b) { return (unsigned int)(yy * sw + word * 64 + b); };
    bool ok = true;
    {
        const unsigned long long UW = W & Wp & J, UB = B & Bp & J;
        if (UW & ~(UW << 1) & bit) ok &= seg_global_join(P, gidx(wx, y, seg_start_of(seg_starts(W, J), bx)), gidx(wx, y - 1, seg_start_of(seg_starts(Wp, J), bx)));
        if (UB & ~(UB << 1) & bit) ok &= seg_global_join(P, gidx(wx, y, seg_start_of(seg_starts(B, J), bx)), gidx(wx, y - 1, seg_start_of(seg_starts(Bp, J), bx)));
    }
    if (W & J & bit) {
        // white diagonals, where "up" does not already make the connection; at the ends of the word they reach into the
        // neighbouring words of the row above
        const unsigned int me = gidx(wx, y, seg_start_of(seg_starts(W, J), bx));
        if (!((Wp >> bx) & 1ull)) {
            if (bx > 0) {
                if ((Wp >> (bx - 1)) & 1ull) ok &= seg_global_join(P, me, gidx(wx, y - 1, seg_start_of(seg_starts(Wp, J), bx - 1)));
            } else if (wx > 0) {
                const unsigned long long Wlp = wm[m0 - sh - 1];
                if (Wlp >> 63) ok &= seg_global_join(P, me, gidx(wx - 1, y - 1, seg_start_of(seg_starts(Wlp, seg_join_mask(x0 - 64, sw)), 63)));
            }
        }
        // up-right is redundant only if up connects AND pixel x+1 of the row above joins pixel x there
        if (bx < 63) {
            if (((Wp >> (bx + 1)) & 1ull) && !(((Wp >> bx) & 1ull) && ((J >> (bx + 1)) & 1ull)))
                ok &= seg_global_join(P, me, gidx(wx, y - 1, seg_start_of(seg_starts(Wp, J), bx + 1)));
        } else if (wx + 1 < nwx) {
            const unsigned long long Wrp = wm[m0 + sh - 1];
            if ((Wrp & 1ull) && !((Wp >> 63) && (seg_join_mask(x0 + 64, sw) & 1ull))) ok &= seg_global_join(P, me, gidx(wx + 1, y - 1, 0));
        }
    }
    if (!ok) atomicAdd((unsigned long long *)&counters[CNT_UF_GUARD], 1ull);
}

// Both kinds of seam in one launch (they are independent of each other and both are chains of L2 round trips: side by
// side their latencies overlap): the first ncol_blocks workgroups take the word seams, the others the row seams.
__global__ void __launch_bounds__(64) k_seg_border(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                   const uint4 *__restrict__ edges, int ntiles, Geom g, int nwx, unsigned int *__restrict__ parent,
                                                   long long *counters, unsigned int ncol_blocks, int nrb)
{
    if (blockIdx.x < ncol_blocks) {
        seg_border_cols_body(wmask, bmask, edges, ntiles, g, nwx, parent, counters, blockIdx.x);
    } else {
        const unsigned int r = blockIdx.x - ncol_blocks;
        const unsigned int t = r / (unsigned int)nwx;
        seg_border_rows_body(wmask, bmask, g, nwx, parent, counters, (int)(r - t * (unsigned int)nwx), (int)(t % (unsigned int)nrb), (int)(t / (unsigned int)nrb));
    }
}

// Tile-local roots -> global roots (the rootmask here is laid out [frame][word column][row]).
__global__ void __launch_bounds__(256) k_seg_roots(const unsigned long long *__restrict__ rootmask, Geom g, int nwx,
                                                   unsigned int *__restrict__ parent, unsigned int *__restrict__ sizes)
{
    const size_t per_frame = (size_t)nwx * g.sh;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_frame * g.nframes) return;
    unsigned long long w = rootmask[i];
    if (!w) return;
    const int fr = (int)(i / per_frame);
    const int rem = (int)(i - (size_t)fr * per_frame);
    const int wx = rem / g.sh, y = rem - wx * g.sh;
    unsigned int *P = parent + (size_t)fr * g.npix;
    unsigned int *S = sizes + (size_t)fr * g.npix;
    while (w) {
        const int b = __ffsll((long long)w) - 1;
        w &= w - 1;
        const unsigned int p = (unsigned int)(y * g.sw + wx * 64 + b);
        const unsigned int sp = S[p];  // in flight beside the find
        const unsigned int root = uf_find(P, p);
        if (root != p) {
            atomicAdd(&S[root], sp);
            P[p] = root;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// S4 on masks: the point pass, k_seg_points (K7).
#define SEGP_NSLOT 256          /* slots of the workgroup's cluster table; the last one = "table full": the point probes the global table itself */
#define SEGP_NW 4               /* word columns (wavefronts) of a common-launch workgroup */
#define SEGP_RUNCAP 2048        /* runs a common-launch workgroup stages (4 tiles) */
#define SEGP_RUNCAP_DENSE 4352  /* the maximum of one tile: 64 rows x (64 runs + 2 neighbour pixels) */
#define SEGP_PCAP 4096          /* points a common-launch workgroup parks (4 tiles) */
#define SEGP_PCAP_DENSE 8192    /* the maximum of half a tile: 32 rows x 64 pixels x 4 sites */

// ---- Packed words.  Each of the four formats is stated here and nowhere else (fields from bit 0 up); the asserts hold
// every field against the largest value it must carry.
constexpr bool segp_fits(long long largest, int bits) { return largest < (1ll << bits); }

// Run entry (RT before the labels replace it): start bit 6 | row 6 | kind 2 | tile (wavefront) 2.  An own run starts at
// its start bit of the tile's word; the left neighbour pixel x0-1 carries the start bit of its run in the word on the left,
// the right neighbour pixel x0+64 is bit 0 of the word on the right and starts its run there.
enum : unsigned int { SEGP_RUN_OWN = 0u, SEGP_RUN_LEFT = 1u, SEGP_RUN_RIGHT = 2u };
#define SEGP_RUN_NONE 0xFFFFFFFFu /* no entry (past the end of the list) */
static_assert(segp_fits(SEGP_NW - 1, 2), "run entry: tile");
static_assert(segp_fits(SEG_PH, 6), "row (here and in the item and the parked point): a tile stages rows 0 .. SEG_PH");
__device__ __forceinline__ unsigned int segp_run_tag(int row, int wave) { return ((unsigned int)row << 6) | ((unsigned int)wave << 14); }
__device__ __forceinline__ unsigned int segp_run_pack(unsigned int tag, unsigned int kind, int sx) { return tag | (kind << 12) | (unsigned int)sx; }
__device__ __forceinline__ int segp_run_sx(unsigned int e) { return (int)(e & 63u); }
__device__ __forceinline__ int segp_run_row(unsigned int e) { return (int)((e >> 6) & 63u); }
__device__ __forceinline__ unsigned int segp_run_kind(unsigned int e) { return (e >> 12) & 3u; }
__device__ __forceinline__ int segp_run_wave(unsigned int e) { return (int)((e >> 14) & 3u); }
// x of the entry's run start relative to its own tile's x0
__device__ __forceinline__ int segp_run_dx(unsigned int e)
{
    const unsigned int kind = segp_run_kind(e);
    return (kind == SEGP_RUN_LEFT ? -64 : (kind == SEGP_RUN_RIGHT ? 64 : 0)) + segp_run_sx(e);
}

// Run label (RT once the labels are in): global root 31 | component too small 1.  A root is a pixel index of the
// decimated frame, below 2^CLUSTER_LABEL_BITS (make_geom): two of them and the frame number make a cluster key.
#define SEGP_SMALL 0x80000000u
static_assert(CLUSTER_LABEL_BITS <= 31, "run label: the root and the too-small bit share a word");
__device__ __forceinline__ unsigned int segp_label(unsigned int w) { return w & 0x7FFFFFFFu; }

// ROWB, per (tile, row): first entry of the row in RT 13 | own runs 7 | has a left neighbour pixel 1.  The row's entries are
// its own runs in the order of their start bits, then the left neighbour pixel, then the right one.
static_assert(segp_fits(SEGP_RUNCAP_DENSE, 13) && segp_fits(SEGP_RUNCAP, 13), "ROWB: first entry (at most the table's size)");
static_assert(segp_fits(64, 7), "ROWB: own runs of a 64-pixel row");
static_assert(SEGP_RUNCAP_DENSE >= 64 * (64 + 2), "the dense launch stages every run a tile can have");
__device__ __forceinline__ unsigned int segp_rowb_pack(int base, int nown, bool havel) { return (unsigned int)base | ((unsigned int)nown << 13) | (havel ? 1u << 20 : 0u); }
__device__ __forceinline__ int segp_rowb_base(unsigned int rb) { return (int)(rb & 0x1FFFu); }
__device__ __forceinline__ int segp_rowb_own(unsigned int rb) { return (int)((rb >> 13) & 0x7Fu); }
__device__ __forceinline__ int segp_rowb_left(unsigned int rb) { return (int)((rb >> 20) & 1u); }

// The one run lookup: index into RT of the run that holds pixel xx = -1 .. 64 of a row, from the row's ROWB word and
// its run starts S (ROWS).  Pixel xx must belong to a run that was staged.
__device__ __forceinline__ int segp_run_index(unsigned int rb, unsigned long long S, int xx)
{
    const int b = segp_rowb_base(rb), no = segp_rowb_own(rb);
    if (xx < 0) return b + no;
    if (xx > 63) return b + no + segp_rowb_left(rb);
    return b + __popcll(S & seg_upto(xx)) - 1;
}

// Item (PT while the emitting pixels are listed): lx 6 | row 6 | wavefront 2 | sites 4 | pixel is black 1 | index of
// its first point 13.  Row and wavefront together are the pixel's (tile, row) index into ROWS / ROWB.
static_assert(segp_fits(SEGP_PCAP_DENSE - 1, 13) && segp_fits(SEGP_PCAP - 1, 13), "item: first point (an item is stored only if it is below PCAP)");
__device__ __forceinline__ unsigned int segp_item_tag(int row, int wave) { return ((unsigned int)row << 6) | ((unsigned int)wave << 12); }
__device__ __forceinline__ unsigned int segp_item_pack(unsigned int tag, int lx, unsigned int sites, unsigned int black, unsigned int first)
{
    return (unsigned int)lx | tag | (sites << 14) | (black << 18) | (first << 19);
}
__device__ __forceinline__ int segp_item_lx(unsigned int e) { return (int)(e & 63u); }
__device__ __forceinline__ int segp_item_trow(unsigned int e) { return (int)((e >> 6) & 255u); }
__device__ __forceinline__ unsigned int segp_item_sites(unsigned int e) { return (e >> 14) & 15u; }
__device__ __forceinline__ unsigned int segp_item_first(unsigned int e) { return e >> 19; }

// Parked point (PT once the points are grouped): lx 6 | ly 6 | site 2 | pixel is black 1 | wavefront 2 | slot of the
// workgroup's cluster table 8.  Sites: 0 (1,0), 1 (0,1), 2 (-1,1), 3 (1,1).
static_assert(segp_fits(SEGP_NSLOT - 1, 8), "parked point: table slot");
__device__ __forceinline__ unsigned int segp_point_of_item(unsigned int e) { return (e & 0xFFFu) | (((e >> 18) & 1u) << 14) | (((e >> 12) & 3u) << 15); }  // all but site and slot
__device__ __forceinline__ unsigned int segp_point_pack(unsigned int of_item, unsigned int site, unsigned int slot) { return of_item | (site << 12) | (slot << 17); }
__device__ __forceinline__ int segp_point_lx(unsigned int w) { return (int)(w & 63u); }
__device__ __forceinline__ int segp_point_ly(unsigned int w) { return (int)((w >> 6) & 63u); }
__device__ __forceinline__ int segp_point_site(unsigned int w) { return (int)((w >> 12) & 3u); }
__device__ __forceinline__ bool segp_point_black(unsigned int w) { return (w >> 14) & 1u; }
__device__ __forceinline__ int segp_point_wave(unsigned int w) { return (int)((w >> 15) & 3u); }
__device__ __forceinline__ unsigned int segp_point_slot(unsigned int w) { return w >> 17; }

// The packed counter npts: items 16 | points 16, handed out together by one atomic per row.  Neither half can carry
// into the other: the totals of a workgroup are bounded by its pixels.
static_assert(segp_fits(SEGP_NW * SEG_PH * 64, 16), "npts: items of a common-launch workgroup (4 tiles x 63 rows x 64 pixels)");
static_assert(segp_fits(SEGP_NW * SEG_PH * 64 * 4, 16), "npts: points of a common-launch workgroup (4 sites per pixel)");
static_assert(SEGP_PCAP_DENSE >= 32 * 64 * 4, "the dense launch parks every point half a tile can have");

// ---- Storage plan: the workgroup's LDS.  The kernel declares the arrays and builds one SegpStore of them at its top; the
// steps reach them only through it.  "Free after" is the barrier that ends a life; nothing writes the same memory before it.
//
//   array   bytes: common  dense    life                written by                  read by                      free after
//   ROWS           2048    512      run starts of       scan_runs                   group_park, emit's           the tile's end (dense: the barrier
//   ROWB           1024    256      (tile, row)         scan_runs                   fallback                     opening the next tile)
//   RT             8192    17408    1 run entries       list_runs                   label_runs                   label_runs itself: a thread replaces
//                                                                                                                the entries it read, in place
//                                   2 run labels        label_runs                  group_park, emit's fallback  the tile's end
//   PT             16384   32768    1 SML: u64 per (tile, row) at PT[0, 2 NT), the starts of the runs too small; EFL: u32 per (tile, row) at
//                                     PT[2 NT, 3 NT), bit 0 left / bit 1 right neighbour pixel too small
//                                                       scan_runs (zero, behind     delete_small                 the barrier closing clear_tables
//                                                       its barrier), label_runs                                 of the first half
//                                                       (atomicOr, behind the
//                                                       barrier closing list_runs)
//                                   2 items             list_items                  group_park: a round's items  the barrier inside each round of
//                                                                                   go to registers              group_park
//                                   3 parked points     group_park, at or behind    emit                         the barrier opening the next half
//                                                       the items of its round                                   or tile
//   BK             2048    2048     1 cluster key       clear_tables (empty),       reserve                      reserve itself: the thread that read
//   BC             1024    1024       point count       group_park (CAS, add)                                    slot i replaces it
//                                   2 global slot |     reserve                     emit (BC: atomicAdd hands    the barrier opening the next half
//                                     base << 32; next                              out the positions)           or tile
//                                     position
//   npts           4       4        items | points<<16  clear_tables (zero),        group_park                   the barrier opening the next half
//                                                       list_items (atomicAdd)                                   or tile
//   base           4       4        the frame cursor    reserve, before its barrier reserve, behind it           the same
//   wtot           16      4        runs per tile       scan_runs, before its       scan_runs, behind it         the barrier opening the next tile
//                                                       barrier
//   sum            30744   54028
//
// The build reports 31000 B for the common launch (256 B more: the scratch of __syncthreads_or) and 54032 B for the dense
// one (4 B of padding behind the scalars).
template <int PCAP_, int RUNCAP_, int NW_, int NHALF_>
struct SegpStore {
    static constexpr int PCAP = PCAP_, RUNCAP = RUNCAP_, NW = NW_, NHALF = NHALF_, NT = 64 * NW_, NSLOT = SEGP_NSLOT;
    static constexpr bool DENSE = NHALF_ > 1;
    unsigned int *RT;          // [RUNCAP]
    unsigned long long *ROWS;  // [NT]
    unsigned int *ROWB;        // [NT]
    unsigned long long *BK;    // [NSLOT]
    unsigned int *BC;          // [NSLOT]
    unsigned int *PT;          // [PCAP], 8-byte aligned
    unsigned int *npts, *base, *wtot;  // two words and [NW]
    __device__ __forceinline__ unsigned long long *SML() const { return reinterpret_cast<unsigned long long *>(PT); }
    __device__ __forceinline__ unsigned int *EFL() const { return PT + 2 * NT; }
    static_assert(PCAP >= 3 * NT, "the small-run masks borrow the parking space");
};
constexpr size_t segp_lds_bytes(int pcap, int runcap, int nw) { return (size_t)64 * nw * (8 + 4) + SEGP_NSLOT * (8 + 4) + 4 * (size_t)runcap + 4 * (size_t)pcap + 4 * (2 + (size_t)nw); }
static_assert(segp_lds_bytes(SEGP_PCAP, SEGP_RUNCAP, SEGP_NW) + 256 == 31000, "common launch: the plan and the LDS the build reports disagree");
static_assert(segp_lds_bytes(SEGP_PCAP_DENSE, SEGP_RUNCAP_DENSE, 1) + 4 == 54032, "dense launch: the plan and the LDS the build reports disagree");

// where the wavefront's tile lies
struct SegpTile {
    int fr, wx, x0, y0;
    int xg0;          // x0 of the workgroup's first tile (the tile of wavefront w starts at xg0 + 64 w)
    unsigned int id;  // (frame * tiles_y + tile_y) * nwx + word column, as the dense-tile list holds it
};
// what a lane holds of its row (lane = row of the tile)
struct SegpRow {
    unsigned long long W, B;  // the row's masks; segp_delete_small takes the runs of small components out
    unsigned int nb;          // pixel x0-1 of the row is white 1 | black 2, pixel x0+64 white 4 | black 8 (the same deletion applies)
    unsigned long long SL;    // run starts of the left neighbour pixel's colour in its word
    __device__ __forceinline__ bool wl() const { return nb & 1u; }
    __device__ __forceinline__ bool bl() const { return nb & 2u; }
    __device__ __forceinline__ bool wr() const { return nb & 4u; }
    __device__ __forceinline__ bool br() const { return nb & 8u; }
    __device__ __forceinline__ bool havel() const { return nb & 3u; }
    __device__ __forceinline__ bool haver() const { return nb & 12u; }
};
struct SegpRuns { unsigned long long Sall; int base, total; };  // the row's run starts (both colours), its first entry in RT, the workgroup's entries
// the masks of the neighbours of pixel x, aligned to bit x, after the deletion: n = (x, y+1), sr = (x+1, y), nsr = (x+1, y+1), nsl = (x-1, y+1)
struct SegpNbr { unsigned long long Wn, Bn, Wsr, Bsr, Wnsr, Bnsr, Wnsl, Bnsl; };
// where the points go: the global cluster table and the per-frame staging rows
struct SegpOut {
    unsigned long long *keys;
    unsigned int *counts, hmask;
    unsigned long long *stage_rec;
    unsigned int *stage_pos, *frame_cursor, stage_cap;
    long long *counters;
};
// What a step tells the kernel body, which alone acts on it (the rule stands above k_seg_points)
enum SegpStatus { SEGP_GO, SEGP_SKIP_HALF, SEGP_OVER_CAPACITY };

// ---- The steps.  Each header says what the step reads and writes (SegpStore members, the lane's registers) and whether it
// ends with a workgroup barrier.

// Load: the masks of the lane's row and the pixels x0-1 and x0+64 beside it, from global memory.  No barrier.
__device__ __forceinline__ SegpRow segp_load_row(const unsigned long long *wm, const unsigned long long *bm, const SegpTile &T, int y, int nwx, int sw, int sh)
{
    SegpRow R = {0ull, 0ull, 0u, 0ull};
    if (y < sh && T.wx < nwx) {
        const size_t m0 = (size_t)T.wx * sh + y;
        R.W = wm[m0]; R.B = bm[m0];
        if (T.wx > 0) {
            const unsigned long long Wl = wm[m0 - sh], Bl = bm[m0 - sh];
            R.nb = (unsigned int)(Wl >> 63) | ((unsigned int)(Bl >> 63) << 1);
            if (R.havel()) R.SL = seg_starts(R.wl() ? Wl : Bl, seg_join_mask(T.x0 - 64, sw));
        }
        if (T.wx + 1 < nwx) R.nb |= (((unsigned int)wm[m0 + sh] & 1u) << 2) | (((unsigned int)bm[m0 + sh] & 1u) << 3);
    }
    return R;
}

// Count and scan runs: every row's entries (own runs + neighbour pixels; none for a tile without contrast) are summed over
// the rows and the tiles.  Writes wtot, then BARRIER, then ROWS, ROWB and zeroes SML / EFL; no barrier at the end (list_runs
// closes with one).  SEGP_OVER_CAPACITY: the workgroup has more entries than RT holds.
template <class ST>
__device__ __forceinline__ SegpStatus segp_scan_runs(const ST &st, const SegpRow &R, unsigned long long J, bool tile_live, int tid, SegpRuns &Q)
{
    const int lane = tid & 63, wid = tid >> 6;
    Q.Sall = seg_starts(R.W, J) | seg_starts(R.B, J);
    const int nown = __popcll(Q.Sall);
    const int cnt = tile_live ? nown + (R.havel() ? 1 : 0) + (R.haver() ? 1 : 0) : 0;
    int incl = cnt;  // inclusive prefix over the rows, then over the tiles
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) st.wtot[wid] = (unsigned int)incl;
    __syncthreads();
    Q.base = incl - cnt; Q.total = 0;
#pragma unroll
    for (int w = 0; w < ST::NW; w++) {
        if (w < wid) Q.base += (int)st.wtot[w];
        Q.total += (int)st.wtot[w];
    }
    st.SML()[tid] = 0ull;
    st.EFL()[tid] = 0u;
    st.ROWS[tid] = Q.Sall;
    st.ROWB[tid] = segp_rowb_pack(Q.base, nown, R.havel());
    return !ST::DENSE && Q.total > ST::RUNCAP ? SEGP_OVER_CAPACITY : SEGP_GO;  // the dense launch holds the maximum (asserted above)
}

// List runs: the row's lane writes its run entries to RT[base ..].  Ends with a BARRIER.
template <class ST>
__device__ __forceinline__ void segp_list_runs(const ST &st, const SegpRow &R, const SegpRuns &Q, bool tile_live, int tid)
{
    if (tile_live) {
        unsigned long long m = Q.Sall;
        int j = Q.base;
        const unsigned int tag = segp_run_tag(tid & 63, tid >> 6);
        while (m) {
            const int sx = __ffsll((long long)m) - 1;
            m &= m - 1;
            st.RT[j++] = segp_run_pack(tag, SEGP_RUN_OWN, sx);
        }
        if (R.havel()) st.RT[j++] = segp_run_pack(tag, SEGP_RUN_LEFT, seg_start_of(R.SL, 63));
        if (R.haver()) st.RT[j++] = segp_run_pack(tag, SEGP_RUN_RIGHT, 0);
    }
    __syncthreads();
}

// Label runs, one run per thread and step: run start -> tile-local root -> global root -> size, from global memory (each
// level issued for four runs per thread before waiting).  Reads RT (run entries) and replaces them by the labels; marks
// the runs of components below MIN_COMPONENT in SML / EFL.  Ends with a BARRIER.
template <class ST>
__device__ __forceinline__ void segp_label_runs(const ST &st, const SegpTile &T, const unsigned int *lab, const unsigned int *siz, int sw, int total, int tid)
{
    for (int i0 = 0; i0 < total; i0 += 4 * ST::NT) {
        unsigned int e[4], l[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * ST::NT + tid;
            e[u] = i < total ? st.RT[i] : SEGP_RUN_NONE;
            const int ex0 = T.xg0 + (ST::DENSE ? 0 : segp_run_wave(e[u])) * 64;
            const unsigned int p = (unsigned int)((T.y0 + segp_run_row(e[u])) * sw + ex0 + segp_run_dx(e[u]));
            l[u] = e[u] != SEGP_RUN_NONE ? lab[p] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) l[u] = e[u] != SEGP_RUN_NONE ? lab[l[u]] : 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) s[u] = e[u] != SEGP_RUN_NONE ? siz[l[u]] : MIN_COMPONENT;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * ST::NT + tid;
            if (e[u] == SEGP_RUN_NONE) continue;
            const bool small = s[u] < MIN_COMPONENT;
            st.RT[i] = l[u] | (small ? SEGP_SMALL : 0u);
            if (small) {
                const int trow = segp_run_row(e[u]) + 64 * segp_run_wave(e[u]);
                if (segp_run_kind(e[u]) == SEGP_RUN_OWN) {
                    const int sx = segp_run_sx(e[u]);
                    atomicOr(reinterpret_cast<unsigned int *>(&st.SML()[trow]) + (sx >> 5), 1u << (sx & 31));
                } else
                    atomicOr(&st.EFL()[trow], segp_run_kind(e[u]));  // SEGP_RUN_LEFT = bit 0, SEGP_RUN_RIGHT = bit 1
            }
        }
    }
    __syncthreads();
}

// Delete small runs: a run of a component with fewer than 25 pixels behaves like "no contrast" and leaves the lane's masks
// (R.W, R.B, the neighbour pixels).  Reads SML / EFL; returns the neighbours' masks the four sites are made of, taken after
// the deletion (the row below is lane + 1).  No barrier.
template <class ST>
__device__ __forceinline__ SegpNbr segp_delete_small(const ST &st, SegpRow &R, unsigned long long J, int tid)
{
    unsigned long long m = st.SML()[tid];
    while (m) {
        const int sx = __ffsll((long long)m) - 1;
        m &= m - 1;
        const bool white = (R.W >> sx) & 1ull;
        const int len = seg_run_len(white ? R.W : R.B, J, sx);
        const unsigned long long bits = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << sx;
        if (white) R.W &= ~bits; else R.B &= ~bits;
    }
    const unsigned int ef = st.EFL()[tid];
    if (ef & 1u) R.nb &= ~3u;
    if (ef & 2u) R.nb &= ~12u;
    SegpNbr N;
    N.Wn = __shfl_down(R.W, 1); N.Bn = __shfl_down(R.B, 1);
    const int fln = __shfl_down((int)R.nb, 1);
    const bool wln = fln & 1, bln = fln & 2, wrn = fln & 4, brn = fln & 8;
    N.Wsr = (R.W >> 1) | ((unsigned long long)R.wr() << 63); N.Bsr = (R.B >> 1) | ((unsigned long long)R.br() << 63);
    N.Wnsr = (N.Wn >> 1) | ((unsigned long long)wrn << 63); N.Bnsr = (N.Bn >> 1) | ((unsigned long long)brn << 63);
    N.Wnsl = (N.Wn << 1) | (unsigned long long)wln; N.Bnsl = (N.Bn << 1) | (unsigned long long)bln;
    return N;
}

// Site masks: E[k] bit x = pixel x of the row emits the point of site k (0 (1,0), 1 (0,1), 2 (-1,1), 3 (1,1): one pixel
// white, the other black), for the emitting pixels V of this half.  Registers only.
__device__ __forceinline__ void segp_site_masks(const SegpRow &R, const SegpNbr &N, unsigned long long V, int x0, unsigned long long (&E)[4])
{
    E[0] = ((R.W & N.Bsr) | (R.B & N.Wsr)) & V;
    E[1] = ((R.W & N.Bn) | (R.B & N.Wn)) & V;
    E[3] = ((R.W & N.Bnsr) | (R.B & N.Wnsr)) & V;
    E[2] = ((R.W & N.Bnsl) | (R.B & N.Wnsl)) & V;
    // the (-1,1) point of pixel x is the (1,1) point of pixel x-1: dropped when x-1 emitted it (x-1 >= 1)
    unsigned long long cl = E[3] << 1;
    if (x0 >= 64 && ((R.wl() && (N.Bn & 1ull)) || (R.bl() && (N.Wn & 1ull)))) cl |= 1ull;  // pixel x0-1 is an emitting pixel of the same row range
    E[2] &= ~cl;
}

// Clear tables: empties BK / BC and zeroes npts for a half.  Ends with a BARRIER.
template <class ST>
__device__ __forceinline__ void segp_clear_tables(const ST &st, int tid)
{
    if (tid == 0) *st.npts = 0;
    for (int i = tid; i < ST::NSLOT; i += ST::NT) { st.BK[i] = HASH_EMPTY; st.BC[i] = 0; }
    __syncthreads();
}

// List items.  A row's lane only LISTS its emitting pixels (a short loop without a dependent memory access); the label
// look-ups and the table probes are then done one pixel per thread, by all threads of the workgroup, however the pixels
// are spread over the rows (a tag covers a third of a tile's rows and its payload rows hold most of the pixels).  The list
// lives in the parking space itself: one packed counter (npts) hands out item and point indices together, so an item's
// points are parked at or behind the item's own place, and the rounds of group_park run from the end of the list.
// Reads the site masks and R.B; writes PT (items) and npts.  Ends with a BARRIER.
template <class ST>
__device__ __forceinline__ void segp_list_items(const ST &st, const SegpRow &R, const unsigned long long (&E)[4], int tid)
{
    const unsigned long long any = E[0] | E[1] | E[2] | E[3];
    const unsigned int npts_lane = (unsigned int)(__popcll(E[0]) + __popcll(E[1]) + __popcll(E[2]) + __popcll(E[3]));
    const unsigned int nitems_lane = (unsigned int)__popcll(any);
    unsigned int ib = 0, pi = 0;
    if (nitems_lane) {
        const unsigned int old = atomicAdd(st.npts, nitems_lane | (npts_lane << 16));
        ib = old & 0xFFFFu; pi = old >> 16;
    }
    const unsigned int rowtag = segp_item_tag(tid & 63, tid >> 6);
    // the two 32-pixel halves of the word one after the other: every step of the walk is a 32-bit operation
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        unsigned int a = (unsigned int)(any >> (32 * hf));
        const unsigned int e0 = (unsigned int)(E[0] >> (32 * hf)), e1 = (unsigned int)(E[1] >> (32 * hf)), e2 = (unsigned int)(E[2] >> (32 * hf)),
                           e3 = (unsigned int)(E[3] >> (32 * hf)), bb = (unsigned int)(R.B >> (32 * hf));
        while (a) {
            const int b = __ffs((int)a) - 1;
            a &= a - 1;
            const unsigned int m = ((e0 >> b) & 1u) | (((e1 >> b) & 1u) << 1) | (((e2 >> b) & 1u) << 2) | (((e3 >> b) & 1u) << 3);
            if (pi < (unsigned int)ST::PCAP) st.PT[ib] = segp_item_pack(rowtag, b + 32 * hf, m, (bb >> b) & 1u, pi);
            ib++;
            pi += (unsigned int)__popc(m);
        }
    }
    __syncthreads();
}

// Group items and park points: one item per thread and round; the labels of the pixel and of its up to four partners come
// from ROWB / ROWS / RT, every (pixel, partner label) pair is looked up or entered in BK, counted in BC, and the pixel's
// points are parked in PT with the slot.  A round's items are in registers before the round's first point is parked (the
// barrier inside the round).  npts = the half's points.  Ends with a BARRIER.  SEGP_OVER_CAPACITY: more points than PT
// holds (nothing was parked); SEGP_SKIP_HALF: no points.
template <class ST>
__device__ __forceinline__ SegpStatus segp_group_park(const ST &st, int fr, int tid, unsigned int &npts)
{
    constexpr int NSLOT = ST::NSLOT;
    const unsigned int packed = *st.npts;
    const unsigned int nitems = packed & 0xFFFFu;
    npts = packed >> 16;
    if (npts <= (unsigned int)ST::PCAP && nitems > 0) {
#pragma unroll 1
        for (int rd = (int)((nitems - 1u) / (unsigned int)ST::NT); rd >= 0; rd--) {
            const unsigned int i = (unsigned int)rd * (unsigned int)ST::NT + (unsigned int)tid;
            const bool have = i < nitems;
            const unsigned int e = have ? st.PT[i] : 0u;
            __syncthreads();  // every item of the round is in a register before the first point of the round is parked
            if (!have) continue;
            const int lx = segp_item_lx(e), trow = segp_item_trow(e);
            unsigned int m = segp_item_sites(e), pidx = segp_item_first(e);
            // the two rows' tables first, then all run-table reads together
            const unsigned int rb0 = st.ROWB[trow], rb1 = st.ROWB[trow + 1];
            const unsigned long long S0 = st.ROWS[trow], S1 = st.ROWS[trow + 1];
            const int j0 = segp_run_index(rb0, S0, lx);
            const int j00 = segp_run_index(rb0, S0, lx + 1), j10 = segp_run_index(rb1, S1, lx);          // sites 0 (1,0) and 1 (0,1)
            const int j11 = segp_run_index(rb1, S1, lx - 1), j12 = segp_run_index(rb1, S1, lx + 1);      // sites 2 (-1,1) and 3 (1,1)
            const unsigned int rep0 = segp_label(st.RT[j0]);
            unsigned int rep1[4];
            rep1[0] = segp_label(st.RT[(m & 1u) ? j00 : j0]);
            rep1[1] = segp_label(st.RT[(m & 2u) ? j10 : j0]);
            rep1[2] = segp_label(st.RT[(m & 4u) ? j11 : j0]);
            rep1[3] = segp_label(st.RT[(m & 8u) ? j12 : j0]);
            const unsigned int where = segp_point_of_item(e);
            while (m) {
                // the lowest remaining site and every other remaining site with the same neighbour label
                const unsigned int rr = (m & 1u) ? rep1[0] : ((m & 2u) ? rep1[1] : ((m & 4u) ? rep1[2] : rep1[3]));
                const unsigned int grp = m & ((rep1[0] == rr ? 1u : 0u) | (rep1[1] == rr ? 2u : 0u) | (rep1[2] == rr ? 4u : 0u) | (rep1[3] == rr ? 8u : 0u));
                m &= ~grp;
                const unsigned int hi = rep0 > rr ? rep0 : rr, lo = rep0 > rr ? rr : rep0;
                const unsigned long long key = ((unsigned long long)fr << 48) | ((unsigned long long)hi << CLUSTER_LABEL_BITS) | lo;  // == cluster_key(fr, rep0, rr)
                unsigned int h = hi ^ ((lo << 11) | (lo >> 21));
                h ^= h >> 15;
                h ^= h >> 7;
                h &= (unsigned int)(NSLOT - 1);
                if (h == (unsigned int)(NSLOT - 1)) h = (unsigned int)(NSLOT / 2 - 1);  // homes 0 .. NSLOT-2
                unsigned int slot = NSLOT - 1;  // "table full"
#pragma unroll 1
                for (int probe = 0; probe < NSLOT - 1; probe++) {
                    unsigned long long cur = __hip_atomic_load(&st.BK[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == key) { slot = h; break; }
                    if (cur == HASH_EMPTY) {
                        unsigned long long old = atomicCAS(&st.BK[h], HASH_EMPTY, key);
                        if (old == HASH_EMPTY || old == key) { slot = h; break; }
                    }
                    h = h + 1 == (unsigned int)(NSLOT - 1) ? 0u : h + 1;
                }
                if (slot != (unsigned int)(NSLOT - 1)) atomicAdd(&st.BC[slot], (unsigned int)__popc(grp));
#pragma unroll
                for (unsigned int k = 0; k < 4; k++)
                    if (grp & (1u << k)) st.PT[pidx++] = segp_point_pack(where, k, slot);
            }
        }
    }
    __syncthreads();
    if (npts > (unsigned int)ST::PCAP) return SEGP_OVER_CAPACITY;
    return npts == 0 ? SEGP_SKIP_HALF : SEGP_GO;
}

// Reserve: one global table probe + one counted atomic per (workgroup, cluster) -- BK / BC change from (key, count) to
// (global slot | base position << 32, 0) -- and one cursor atomic per workgroup (base).  Ends with a BARRIER.
// SEGP_SKIP_HALF: the frame's staging rows are full (counted in CNT_OVERFLOW_POINTS: the host re-runs the batch).
template <class ST>
__device__ __forceinline__ SegpStatus segp_reserve(const ST &st, const SegpOut &out, int fr, unsigned int npts, int tid, unsigned int &tbase)
{
    for (int i = tid; i < ST::NSLOT - 1; i += ST::NT) {
        const unsigned int c = st.BC[i];
        if (c) {
            int gslot = hash_insert(out.keys, out.hmask, st.BK[i]);
            unsigned int bg = 0xFFFFFFFFu, bb = 0u;
            if (gslot < 0) atomicAdd((unsigned long long *)&out.counters[CNT_OVERFLOW_HASH], 1ull);
            else { bg = (unsigned int)gslot; bb = atomicAdd(&out.counts[gslot], c); }
            st.BK[i] = (unsigned long long)bg | ((unsigned long long)bb << 32);
            st.BC[i] = 0u;
        }
    }
    if (tid == ST::NT - 1) {
        unsigned int b = atomicAdd(&out.frame_cursor[fr], npts);
        if (b + npts > out.stage_cap) { atomicAdd((unsigned long long *)&out.counters[CNT_OVERFLOW_POINTS], 1ull); b = 0xFFFFFFFFu; }
        *st.base = b;
    }
    __syncthreads();
    tbase = *st.base;
    return tbase == 0xFFFFFFFFu ? SEGP_SKIP_HALF : SEGP_GO;
}

// Emit: the parked points leave as dense, coalesced rows: (record | global slot << 36, position in the cluster).  Reads PT
// (parked points), BK / BC (global slot, base, next position); a point whose slot is "table full" finds its two labels
// through the run lookup and probes the global table on its own.  No barrier.
template <class ST>
__device__ __forceinline__ void segp_emit(const ST &st, const SegpOut &out, const SegpTile &T, unsigned int npts, unsigned int tbase, int tid)
{
    uint2 *const srec = reinterpret_cast<uint2 *>(out.stage_rec) + ((size_t)T.fr * out.stage_cap + tbase);
    unsigned int *const spos = out.stage_pos + ((size_t)T.fr * out.stage_cap + tbase);
    for (unsigned int i = tid; i < npts; i += ST::NT) {
        const unsigned int w = st.PT[i];
        const int lx = segp_point_lx(w), ly = segp_point_ly(w), k = segp_point_site(w), pw = segp_point_wave(w);
        const bool black = segp_point_black(w);
        const unsigned int slot = segp_point_slot(w);
        const int dx = k == 0 ? 1 : (k == 1 ? 0 : (k == 2 ? -1 : 1)), dy = k == 0 ? 0 : 1;
        const int px0 = T.xg0 + (ST::DENSE ? 0 : pw) * 64;
        unsigned int gslot, pos;
        if (slot == (unsigned int)(ST::NSLOT - 1)) {  // the table was full
            const int t0 = pw * 64 + ly, t1 = t0 + dy;
            const unsigned int a = segp_label(st.RT[segp_run_index(st.ROWB[t0], st.ROWS[t0], lx)]);
            const unsigned int b = segp_label(st.RT[segp_run_index(st.ROWB[t1], st.ROWS[t1], lx + dx)]);
            int gs = hash_insert(out.keys, out.hmask, cluster_key(T.fr, a, b));
            gslot = gs < 0 ? 0xFFFFFFFFu : (unsigned int)gs;
            pos = gs < 0 ? 0u : atomicAdd(&out.counts[gs], 1u);
            if (gs < 0) atomicAdd((unsigned long long *)&out.counters[CNT_OVERFLOW_HASH], 1ull);
        } else {
            const unsigned long long gb = st.BK[slot];
            gslot = (unsigned int)gb;
            pos = (unsigned int)(gb >> 32) + atomicAdd(&st.BC[slot], 1u);
        }
        const bool good = gslot != 0xFFFFFFFFu;  // table overflow: the place pass skips the record, the batch is re-run
        // == pack_point(2x+dx, 2y+dy, dx*d, dy*d) | gslot << POINT_BITS with d = +255 for a black pixel, -255 for a white one
        const unsigned int cpos = black ? 1u : 2u, cneg = 3u - cpos;
        const unsigned int cgx = dx == 0 ? 0u : (dx > 0 ? cpos : cneg), cgy = dy == 0 ? 0u : cpos;
        uint2 rec;
        rec.x = good ? ((unsigned int)(2 * (px0 + lx) + dx) | ((unsigned int)(2 * (T.y0 + ly) + dy) << 16)) : 0xFFFFFFFFu;
        rec.y = good ? (cgx | (cgy << 2) | (gslot << (POINT_BITS - 32))) : 0xFFFFFFFFu;
        srec[i] = rec;
        spos[i] = good ? pos : 0u;
    }
}

// the wavefront's tile joins the list the dense launch works off
__device__ __forceinline__ void segp_hand_over(unsigned int *dense_tiles, long long *counters, unsigned int tile_id)
{
    dense_tiles[atomicAdd((unsigned long long *)&counters[CNT_DENSE_TILES], 1ull)] = tile_id;
}

// A tile is one word column x 63 emitting rows, one wavefront, lane = row (row 63 only serves as "the row below").  The
// common launch (NW = 4, NHALF = 1) puts four horizontally adjacent tiles in a workgroup that shares the run table, the
// cluster table and the parking space (a dense tile borrows from its sparse neighbours; a cluster that spans the tiles
// costs one global probe, not four); the dense launch (NW = 1, full capacities, a tile emitted in NHALF = 2 halves of rows)
// works off the dense-tile list, one tile per workgroup and trip.
//
// The handover rule, stated here once and acted on only in this body.  A step that finds more runs than RUNCAP or more
// points than PCAP answers SEGP_OVER_CAPACITY:
//   common launch  every tile of the workgroup that has contrast goes on dense_tiles, and the workgroup ends;
//   dense launch   cannot happen (RUNCAP and PCAP are the maxima of a tile and of half a tile, asserted above; the run
//                  check is not even compiled); if points still overflow, CNT_OVERFLOW_POINTS counts it and the half is
//                  skipped.
// SEGP_SKIP_HALF (no points, or the frame's staging rows are full) goes on to the next half or tile.  Every exit passes
// PHASE_FLUSH.
template <int PCAP, int RUNCAP, int NW, int NHALF>
__global__ void __launch_bounds__(64 * NW) k_seg_points(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                        Geom g, int nwx, const unsigned int *__restrict__ labels, const unsigned int *__restrict__ sizes,
                                                        unsigned long long *keys, unsigned int *counts, unsigned int hmask,
                                                        unsigned long long *stage_rec, unsigned int *stage_pos, unsigned int *frame_cursor,
                                                        unsigned int stage_cap, unsigned int *dense_tiles, int tiles_y, long long *counters)
{
    constexpr bool DENSE = NHALF > 1;
    using ST = SegpStore<PCAP, RUNCAP, NW, NHALF>;
    __shared__ unsigned int RT[RUNCAP];
    __shared__ unsigned long long ROWS[ST::NT];
    __shared__ unsigned int ROWB[ST::NT];
    __shared__ unsigned long long BK[ST::NSLOT];
    __shared__ unsigned int BC[ST::NSLOT];
    __shared__ __attribute__((aligned(8))) unsigned int PT[PCAP];
    __shared__ unsigned int s_npts, s_base, s_wtot[NW];
    static_assert(sizeof RT + sizeof ROWS + sizeof ROWB + sizeof BK + sizeof BC + sizeof PT + sizeof s_npts + sizeof s_base + sizeof s_wtot == segp_lds_bytes(PCAP, RUNCAP, NW),
                  "the arrays declared here are the plan's");
    const ST st = {RT, ROWS, ROWB, BK, BC, PT, &s_npts, &s_base, s_wtot};
    const SegpOut out = {keys, counts, hmask, stage_rec, stage_pos, frame_cursor, stage_cap, counters};
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int sw = g.sw, sh = g.sh;
    const size_t per_frame = (size_t)nwx * sh;
    PHASE_DECL();
    const long long ndense = DENSE ? counters[CNT_DENSE_TILES] : 1;
    for (long long work = DENSE ? blockIdx.x : 0; work < ndense; work += DENSE ? gridDim.x : 1) {
        SegpTile T;
        int ty;
        if (DENSE) {
            __syncthreads();  // the previous tile's last reads of the LDS are done
            const unsigned int tile_id = dense_tiles[work];
            T.wx = (int)(tile_id % (unsigned int)nwx);
            ty = (int)((tile_id / (unsigned int)nwx) % (unsigned int)tiles_y);
            T.fr = (int)(tile_id / (unsigned int)(nwx * tiles_y));
        } else {
            // frame-major grid: workgroups that run at the same time belong to different frames, so the per-frame cursor and
            // the per-cluster counters are not hammered by thousands of waves at once (one address sustains ~90 atomics/us)
            T.fr = blockIdx.x; ty = blockIdx.z; T.wx = (int)blockIdx.y * NW + wid;
        }
        T.id = (unsigned int)((T.fr * tiles_y + ty) * nwx + T.wx);
        T.x0 = T.wx * 64; T.y0 = ty * SEG_PH;
        T.xg0 = DENSE ? T.x0 : (int)blockIdx.y * NW * 64;
        const int y = T.y0 + lane;
        PHASE_INIT();
        SegpRow R = segp_load_row(wmask + (size_t)T.fr * per_frame, bmask + (size_t)T.fr * per_frame, T, y, nwx, sw, sh);
        const bool tile_live = __ballot((R.W | R.B) != 0ull) != 0ull;
        if (!DENSE) {
            // most workgroups of a typical frame hold no contrast at all
            if (!__syncthreads_or(tile_live ? 1 : 0)) { PHASE_FLUSH(32); return; }
        }
        const unsigned long long J = seg_join_mask(T.x0, sw);
        SegpRuns Q;
        if (segp_scan_runs(st, R, J, tile_live, tid, Q) == SEGP_OVER_CAPACITY) {
            if (lane == 0 && tile_live) segp_hand_over(dense_tiles, counters, T.id);
            PHASE_FLUSH(32);
            return;
        }
        segp_list_runs(st, R, Q, tile_live, tid);
        PHASE(32);
        segp_label_runs(st, T, labels + (size_t)T.fr * g.npix, sizes + (size_t)T.fr * g.npix, sw, Q.total, tid);
        PHASE(33);
        const SegpNbr N = segp_delete_small(st, R, J, tid);
#pragma unroll 1
        for (int half = 0; half < NHALF; half++) {
            const int rlo = NHALF == 1 ? 0 : half * 32, rhi = NHALF == 1 ? SEG_PH - 1 : min(half * 32 + 31, SEG_PH - 1);
            if (half > 0) __syncthreads();  // the previous half's emit has read PT, BK and BC
            segp_clear_tables(st, tid);
            const unsigned long long V = (lane >= rlo && lane <= rhi && y >= 1 && y <= sh - 2) ? J : 0ull;  // emitting pixels: 1 <= x <= sw-2, 1 <= y <= sh-2
            unsigned long long E[4];
            segp_site_masks(R, N, V, T.x0, E);
            segp_list_items(st, R, E, tid);
            PHASE(37);
            unsigned int npts, tbase;
            SegpStatus s = segp_group_park(st, T.fr, tid, npts);
            PHASE(34);
            if (s == SEGP_OVER_CAPACITY) {
                if (!DENSE) {
                    if (lane == 0 && tile_live) segp_hand_over(dense_tiles, counters, T.id);
                    PHASE_FLUSH(32);
                    return;
                }
                if (tid == 0) atomicAdd((unsigned long long *)&counters[CNT_OVERFLOW_POINTS], 1ull);
                continue;
            }
            if (s == SEGP_SKIP_HALF) continue;
            s = segp_reserve(st, out, T.fr, npts, tid, tbase);
            PHASE(35);
            if (s == SEGP_SKIP_HALF) continue;
            segp_emit(st, out, T, npts, tbase, tid);
            PHASE(36);
        }
    }
    PHASE_FLUSH(32);
}

// ---- introspection for the parity tests (asl_debug_fetch): the byte image and per-pixel labels the oracle reports
__global__ void __launch_bounds__(256) k_seg_debug_thresh(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                          Geom g, int nwx, uint8_t *__restrict__ thresh)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, fr = blockIdx.z;
    if (x >= g.sw || y >= g.sh) return;
    const size_t mi = ((size_t)fr * nwx + (x >> 6)) * g.sh + y;
    const unsigned long long W = wmask[mi], B = bmask[mi];
    thresh[(size_t)fr * g.npix + (size_t)y * g.sw + x] = ((W >> (x & 63)) & 1ull) ? 255 : (((B >> (x & 63)) & 1ull) ? 0 : 127);
}

__global__ void __launch_bounds__(256) k_seg_debug_labels(const unsigned long long *__restrict__ wmask, const unsigned long long *__restrict__ bmask,
                                                          Geom g, int nwx, const unsigned int *__restrict__ parent, unsigned int *__restrict__ out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, fr = blockIdx.z;
    if (x >= g.sw || y >= g.sh) return;
    const int wx = x >> 6, b = x & 63;
    const size_t mi = ((size_t)fr * nwx + wx) * g.sh + y;
    const unsigned long long W = wmask[mi], B = bmask[mi];
    const unsigned int p = (unsigned int)(y * g.sw + x);
    unsigned int l = p;
    if (((W | B) >> b) & 1ull) {
        const unsigned long long J = seg_join_mask(wx * 64, g.sw);
        const unsigned long long S = seg_starts(((W >> b) & 1ull) ? W : B, J);
        l = uf_find(parent + (size_t)fr * g.npix, (unsigned int)(y * g.sw + wx * 64 + seg_start_of(S, b)));
    }
    out[(size_t)fr * g.npix + p] = l;
}
