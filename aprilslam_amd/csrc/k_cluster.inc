// S4: gradient clusters.  Every pair of adjacent pixels with one black and one white pixel,
// both in components of >= 25 pixels, contributes the half-way point (half-pixel fixed point)
// and the direction of the white pixel to the cluster keyed by the two component labels.
//
// Upstream builds per-cluster lists in a hash map; here the work is three flat passes:
//   count   : points -> open-addressing hash table (key = frame|labelHi|labelLo): k_seg_points (k_seg.inc) groups a
//             workgroup's points in a small LDS table first, so that global memory sees one table probe and one counted
//             atomic per (workgroup, cluster)
//   filter  : one thread per table slot applies the size rejection, reserves a contiguous
//             segment of the point pool and files the cluster under its size class
//   scatter : points of surviving clusters are written into their segment as packed records
//             (gy | gx | y | x); the fit kernel derives box, polarity and sort keys from them
// The order in which points/clusters arrive is irrelevant: every later step sorts by key.

__device__ __forceinline__ unsigned long long hash64(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

#define CLUSTER_LABEL_BITS 24 /* a label is a pixel index of the decimated frame: make_geom refuses frames of 2^24 pixels or more */
static_assert(2 * CLUSTER_LABEL_BITS <= 48, "cluster key: two labels below the frame number");

__device__ __forceinline__ unsigned long long cluster_key(int fr, unsigned int a, unsigned int b)
{
    unsigned int hi = a > b ? a : b, lo = a > b ? b : a;
    return ((unsigned long long)fr << 48) | ((unsigned long long)hi << CLUSTER_LABEL_BITS) | lo;
}

// insert-or-find; returns slot or -1 on overflow
__device__ __noinline__ int hash_insert(unsigned long long *keys, unsigned int mask, unsigned long long key)
{
    unsigned int slot = (unsigned int)hash64(key) & mask;
#pragma unroll 1
    for (int probe = 0; probe < HASH_MAX_PROBE; probe++) {
        unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return (int)slot;
        if (cur == HASH_EMPTY) {
            unsigned long long old = atomicCAS(&keys[slot], HASH_EMPTY, key);
            if (old == HASH_EMPTY || old == key) return (int)slot;
        }
        slot = (slot + 1) & mask;
    }
    return -1;
}

// start of a batch: empty cluster table, zeroed batch counters and per-frame cursors (one launch instead of three
// memsets and a kernel)
__global__ void __launch_bounds__(256) k_hash_clear(unsigned long long *keys, unsigned int *counts, unsigned int nslots, long long *counters,
                                                    unsigned int *frame_cursor, unsigned int *frame_ndets, unsigned int nframes)
{
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (unsigned int)CNT__N) counters[i] = 0;
    if (i < nframes) { frame_cursor[i] = 0u; frame_ndets[i] = 0u; }
    if (i >= nslots) return;
    keys[i] = HASH_EMPTY;
    counts[i] = 0;
}

#define POINT_BITS 36  /* packed point record: x(16) y(16) gx(2) gy(2) */

// packed point record: bits 0-15 x, 16-31 y, 32-33 gx code, 34-35 gy code (0: 0, 1: +255, 2: -255); the point pass
// (k_seg_points) assembles it as two 32-bit halves and puts the cluster's table slot above it

// one thread per hash slot; pool allocations are aggregated per 1024-thread block so that each global
// counter sees one atomic per block
__global__ void __launch_bounds__(1024) k_cluster_filter(const unsigned long long *__restrict__ keys, const unsigned int *__restrict__ counts,
                                                         unsigned int nslots, Geom g, ClusterRec *clusters, unsigned long long *slot_seg,
                                                         unsigned int *class_lists, unsigned int max_clusters, unsigned int max_points,
                                                         long long *counters)
{
    __shared__ unsigned int s_keep[16], s_pts[16], s_cls[16][NCLASSES];
    __shared__ unsigned long long s_base_ci, s_base_off, s_base_cls[NCLASSES];
    unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    unsigned long long key = i < nslots ? keys[i] : HASH_EMPTY;
    unsigned int cnt = i < nslots ? counts[i] : 0;
    bool keep = key != HASH_EMPTY && cnt >= 24u && cnt <= 3u * (unsigned int)(2 * g.sw + 2 * g.sh);
    int cls = cnt <= CLASS0_CAP ? 0 : (cnt <= CLASS1_CAP ? 1 : (cnt <= CLASS2_CAP ? 2 : (cnt <= CLASS3_CAP ? 3 : 4)));
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long mask = __ballot(keep);
    unsigned int v = keep ? cnt : 0u, incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    unsigned long long mc[NCLASSES];
#pragma unroll
    for (int c = 0; c < NCLASSES; c++) mc[c] = __ballot(keep && cls == c);
    if (lane == 63) s_pts[wid] = incl;
    if (lane == 0) {
        s_keep[wid] = (unsigned int)__popcll(mask);
#pragma unroll
        for (int c = 0; c < NCLASSES; c++) s_cls[wid][c] = (unsigned int)__popcll(mc[c]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int tk = 0, tp = 0, tc[NCLASSES] = {0};
        for (int w = 0; w < nw; w++) {
            tk += s_keep[w]; tp += s_pts[w];
            for (int c = 0; c < NCLASSES; c++) tc[c] += s_cls[w][c];
        }
        s_base_ci = tk ? atomicAdd((unsigned long long *)&counters[CNT_NCLUSTERS], (unsigned long long)tk) : 0ull;
        s_base_off = tp ? atomicAdd((unsigned long long *)&counters[CNT_NPOINTS], (unsigned long long)tp) : 0ull;
        for (int c = 0; c < NCLASSES; c++)
            s_base_cls[c] = tc[c] ? atomicAdd((unsigned long long *)&counters[CNT_CLASS(c)], (unsigned long long)tc[c]) : 0ull;
    }
    __syncthreads();
    if (i < nslots) slot_seg[i] = ~0ull;  // (offset | count << 32) of the slot's cluster in the point pool, or none
    if (!keep) return;
    unsigned long long ci = s_base_ci + __popcll(mask & lt), off = s_base_off + incl - v, cpos = s_base_cls[cls] + __popcll(mc[cls] & lt);
    for (int w = 0; w < wid; w++) { ci += s_keep[w]; off += s_pts[w]; cpos += s_cls[w][cls]; }
    if (ci >= max_clusters) { atomicAdd((unsigned long long *)&counters[CNT_OVERFLOW_CLUSTERS], 1ull); return; }
    ClusterRec r;
    r.key = key; r.offset = (unsigned int)off; r.count = cnt; r.fill = 0; r.pad = 0;
    if (off + cnt > max_points) {
        atomicAdd((unsigned long long *)&counters[CNT_OVERFLOW_POINTS], 1ull);
        r.count = 0; r.offset = 0;
        clusters[ci] = r;
        return;
    }
    clusters[ci] = r;
    slot_seg[i] = (unsigned long long)(unsigned int)off | ((unsigned long long)cnt << 32);
    class_lists[(size_t)cls * max_clusters + (size_t)cpos] = (unsigned int)ci;
}

// Pass 2: move the staged points of surviving clusters into their segments (coalesced reads).
__global__ void __launch_bounds__(256) k_point_place(const unsigned long long *__restrict__ stage_rec, const unsigned int *__restrict__ stage_pos,
                                                     const unsigned int *__restrict__ frame_cursor, unsigned int stage_cap,
                                                     const unsigned long long *__restrict__ slot_seg,
                                                     unsigned long long *points, const long long *__restrict__ counters)
{
    if (batch_poisoned(counters)) return;
    int fr = blockIdx.y;
    unsigned int n = frame_cursor[fr];
    if (n > stage_cap) n = stage_cap;
    // four points per thread and trip: each level of the chain (record, segment of its slot) is in flight for all four
    const unsigned int stride = gridDim.x * blockDim.x;
    for (unsigned int i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
        unsigned long long rec[4], seg[4];
        unsigned int pos[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const unsigned int i = i0 + u * stride;
            const size_t at = (size_t)fr * stage_cap + (i < n ? i : i0);
            rec[u] = i < n ? stage_rec[at] : ~0ull;
            pos[u] = stage_pos[at];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) seg[u] = rec[u] != ~0ull ? slot_seg[rec[u] >> POINT_BITS] : ~0ull;  // where the slot's cluster lives
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (seg[u] == ~0ull) continue;
            const unsigned int off = (unsigned int)seg[u], cnt = (unsigned int)(seg[u] >> 32);
            if (pos[u] < cnt) points[(size_t)off + pos[u]] = rec[u] & ((1ull << POINT_BITS) - 1ull);
        }
    }
}
