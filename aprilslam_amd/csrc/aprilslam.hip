// libaprilslam.so -- host side of the C ABI declared in include/aprilslam.h.
// gfx950 only.  One asl_detector owns a device workspace sized for its largest batch and
// submits the whole detector (+ optional PnP) as one chain of launches on one HIP stream.
#include "../../include/aprilslam.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "asl_common.h"
#include "tag_standard41h12.inc"
#include "k_wave.inc"

#include "k_threshold.inc"
#include "k_blur.inc"
#include "k_cc.inc"
#include "k_cluster.inc"
#include "k_seg.inc"
#include "k_quad.inc"
#include "k_refine.inc"
#include "k_decode.inc"
#include "k_pnp.inc"
#include "k_dedup.inc"
#include "k_graph.inc"
#include "k_render.inc"
#include "k_rectify.inc"
#include "k_gn.inc"
#include "k_localize.inc"
#include "k_posecov.inc"
#include "k_rig.inc"
#include "k_bundle.inc"
#include "k_calib.inc"
#include "k_rigcal.inc"
#include "k_map.inc"
#include "k_smooth.inc"
#include "k_locate.inc"

static thread_local std::string g_err;

// Optional ROCTX ranges around the stage groups, for `rocprofv3 --marker-trace`: ASL_ROCTX=1 in the
// environment loads the marker library at first use; without it these are two predictable branches.
#include <dlfcn.h>
static struct Markers {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool tried = false;
    void load()
    {
        tried = true;
        const char *e = getenv("ASL_ROCTX");
        if (!e || !*e || *e == '0') return;
        void *h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
} g_markers;
static inline void range_push(const char *name) { if (!g_markers.tried) g_markers.load(); if (g_markers.push) g_markers.push(name); }
static inline void range_pop() { if (g_markers.pop) g_markers.pop(); }

static int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) return fail(ASL_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

#define MAX_STAGES 24

static_assert(FAM_MAX == ASL_MAX_FAMILIES, "asl_common.h and aprilslam.h disagree on the families a detector holds");

struct asl_detector {
    int device = 0;
    int maxhamming = 1;
    int decimate = 2;
    int refine = 1;
    int pnp_both_minima = 0;
    BlurTaps blur{};  // asl_detector_set_quad_sigma; r = 0: off
    struct Family {
        FamilyDev dev;
        int id_base = 0;                             // a tag with local id k is reported as id_base + k (0 for a one-family detector)
        std::vector<unsigned long long> host_codes;  // the family's whole table, the detector's own copy: the index and the id limit read it
        DevBuf<unsigned long long> codes;        // the family's code book (FamilyDev::codes)
        DevBuf<unsigned short> idx_start;        // code-book index of the family (FamilyDev), rebuilt when the id limit changes
        DevBuf<unsigned long long> idx_entries;
    };
    Family fams[ASL_MAX_FAMILIES];
    int nfam = 1;
    DevBuf<FamilyTabDev> fam_tab;  // what k_decode_multi reads, where it is the decoder (decodes_multi, upload_family_table)

    // capacities (grow on overflow)
    unsigned int hash_slots_per_frame = 1024;
    unsigned int clusters_per_frame = 2048;
    unsigned int dets_per_frame = 256;
    double points_per_pixel = 0.5;

    // workspace
    DevBuf<uint8_t> in, dgray, tmin, tmax, tcut;
    DevBuf<uint8_t> bgray;               // k_quad_blur's output; allocated by the first batch that runs with quad_sigma set
    const uint8_t *qgray = nullptr;      // the image the last enqueued batch thresholds and fits on: dgray, or bgray under quad_sigma
    DevBuf<uint8_t> dbg_thresh;         // asl_debug_fetch only: the threshold image as bytes
    DevBuf<unsigned int> dbg_labels;    // asl_debug_fetch only: per-pixel labels
    DevBuf<unsigned int> parent, sizes;
    DevBuf<unsigned long long> hkeys, points, rootmask, wmask, bmask;
    DevBuf<unsigned int> hcounts, class_lists, stage_pos, frame_cursor, dense_tiles, dense_seg, quad_list;
    DevBuf<unsigned long long> stage_rec;
    DevBuf<uint4> seg_edges;  // per labelling tile: its first / last pixel column, a bit per row and colour
    unsigned int stage_cap = 0;  // staged points per frame
    DevBuf<unsigned long long> slot_cluster;  // per hash slot: offset | count << 32 of its cluster's segment
    DevBuf<ClusterRec> clusters;
    DevBuf<QuadRec> quads;
    DevBuf<double> scratch, quadH, wtab, side_mom;  // side_mom: 4 x 6 moments per cluster, k_fit_quads -> k_quad_finish
    DevBuf<DetRec> dets;
    // S8 on the device: per-frame index lists, counts and offsets, and the results in the ABI's layout
    DevBuf<unsigned int> frame_ndets, frame_idx, frame_nkeep, frame_off;
    DevBuf<DetOut> out_det;
    DevBuf<PoseOut> out_pose;
    DevBuf<long long> counters;
    DevBuf<float> pnp_corners;
    DevBuf<double> pnp_out;
    DevBuf<uint8_t> pnp_ok;
    DevBuf<uint8_t> gn_ws;  // asl_gn_solve: its inputs and the LM's buffers (gn_host.inc)
    DevBuf<uint8_t> loc_obs, loc_map;  // the *_batch solver entries: the host records' device copies (grow on demand)
    DevBuf<uint8_t> solve_out;         // the *_batch solver entries: their results, until copied back
    DevBuf<uint8_t> rect_src, rect_dst;  // asl_rectify_u8: the host image's device copy and the result (no batch reads them)
    DevBuf<uint8_t> cal_ws;  // calibration: per-frame workspace and state (k_calib.inc)
    DevBuf<uint8_t> rigcal_ws;  // rig mounting calibration: per-frame workspace, camera tables and state (k_rigcal.inc)
    DevBuf<uint8_t> map_ws, map_lm;  // map reconstruction (k_map.inc): sized by the input / by the problem
    DevBuf<uint8_t> smooth_ws;  // sequence localisation (k_smooth.inc): the chain's and the LM's buffers, sized by n_frames and n_seq
    DevBuf<uint8_t> locate_ws;  // tag location (k_locate.inc): per-id marks, counts and offsets, the view list
    hipStream_t copy_stream = nullptr, host_stream = nullptr;  // host frames: transfers and the chunks' kernels (detect_host_frames)
    std::vector<hipEvent_t> copy_done;
    hipStream_t aux_stream = nullptr;  // highest priority, for the small latency-bound jobs next to a running batch (pose-graph LM)

    // sizes used by the last batch
    Geom last{};
    unsigned int nslots = 0, max_clusters = 0, max_points = 0, max_dets = 0;
    long long last_counters[CNT__N] = {0};
    // batch in flight (asl_submit_batch_device .. asl_collect_batch)
    bool pending = false;
    const uint8_t *p_frames = nullptr;
    Geom p_geom{};
    hipStream_t p_stream = nullptr;
    bool p_has_cam = false;
    CamDev p_cam{};
    size_t prefetched = 0, nd_guess = 0;
    std::chrono::steady_clock::time_point t_submit, t_enqueued;
    PinnedBuf<long long> pinned_counters;  // D2H target that does not force a blocking staging copy
    PinnedBuf<DetOut> host_det;    // pinned staging of the results, grown together with host_pose
    PinnedBuf<PoseOut> host_pose;
    PinnedBuf<unsigned int> host_nkeep;  // per frame

    // profiling
    int profiling = 0;
    hipEvent_t ev[MAX_STAGES + 1] = {nullptr};
    int nev = 0;
    const char *stage_names[MAX_STAGES] = {nullptr};
    float stage_ms[MAX_STAGES] = {0};
    int nstages = 0;
    float host_ms[4] = {0, 0, 0, 0};  // enqueue, wait, copy, post-process of the last batch

    size_t host_cap() const { return std::min(host_det.n, host_pose.n); }  // results the pinned staging holds
    ~asl_detector()  // the buffers free themselves
    {
        for (hipStream_t s : {aux_stream, copy_stream, host_stream})
            if (s) (void)hipStreamDestroy(s);
        for (hipEvent_t e : copy_done) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

static const char *kVersion = "aprilslam 0.1 gfx950 (HIP, tagStandard41h12)";

extern "C" const char *asl_last_error(void) { return g_err.c_str(); }
extern "C" const char *asl_version(void) { return kVersion; }

// Code-book index for k_decode (asl_common.h: FamilyDev): maxhamming + 1 chunks of the code bits; a family wider than 48 bits
// or with more than 65535 ids keeps idx_nch = 0 and is searched as a whole.
static int build_code_index(asl_detector *d, asl_detector::Family &slot)
{
    FamilyDev &f = slot.dev;
    f.idx_nch = 0; f.idx_start = nullptr; f.idx_entries = nullptr;
    const int nch = d->maxhamming + 1;
    if (f.nbits > 48 || f.ncodes > 65535 || nch > IDX_MAX_CHUNKS) return 0;
    if (getenv("ASL_NO_CODE_INDEX")) return 0;  // tests: the search of the whole book must agree with the index
    std::vector<unsigned short> start((size_t)nch * (IDX_BUCKETS + 1), 0);
    std::vector<unsigned long long> entries((size_t)nch * f.ncodes);
    int lo = 0;
    for (int c = 0; c < nch; c++) {
        const int w = f.nbits / nch + (c < f.nbits % nch ? 1 : 0);
        f.idx_lo[c] = lo; f.idx_w[c] = w;
        std::vector<unsigned int> bucket(f.ncodes);
        unsigned short *st = start.data() + (size_t)c * (IDX_BUCKETS + 1);
        for (int i = 0; i < f.ncodes; i++) {
            bucket[i] = idx_bucket((slot.host_codes[i] >> lo) & ((1ull << w) - 1ull), w);
            st[bucket[i] + 1]++;
        }
        for (int b = 0; b < IDX_BUCKETS; b++) st[b + 1] = (unsigned short)(st[b + 1] + st[b]);
        std::vector<unsigned short> fill(st, st + IDX_BUCKETS);
        for (int i = 0; i < f.ncodes; i++)  // ids ascending inside a bucket
            entries[(size_t)c * f.ncodes + fill[bucket[i]]++] = ((unsigned long long)i << 48) | slot.host_codes[i];
        lo += w;
    }
    for (int c = nch; c < IDX_MAX_CHUNKS; c++) { f.idx_lo[c] = 0; f.idx_w[c] = 1; }
    if (slot.idx_start.ensure(start.size()) || slot.idx_entries.ensure((size_t)IDX_MAX_CHUNKS * slot.host_codes.size())) return -1;
    if (hipMemcpy(slot.idx_start.p, start.data(), start.size() * sizeof(unsigned short), hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (hipMemcpy(slot.idx_entries.p, entries.data(), entries.size() * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess) return -1;
    f.idx_start = slot.idx_start.p; f.idx_entries = slot.idx_entries.p; f.idx_nch = nch;
    return 0;
}

// What k_decode and the quad fit assume of a family (k_decode.inc: the storage plan's capacities, rotate90_dev, the packed
// match).  A table that fails here would decode silently wrong, so it never reaches a detector.
extern "C" int asl_family_check(const asl_family *f)
{
    if (!f) return fail(ASL_EINVAL, "family is NULL");
    const int nbits = f->nbits, wb = f->width_at_border, tw = f->total_width;
    if (nbits < 1 || nbits > 63) return fail(ASL_EINVAL, "nbits must be in [1, 63] (got %d)", nbits);
    if (nbits % 4 > 1) return fail(ASL_EINVAL, "nbits %% 4 must be 0 or 1 (got nbits = %d): the rotation search handles nothing else", nbits);
    if (wb < 2 || wb > 8) return fail(ASL_EINVAL, "width_at_border must be in [2, 8] (got %d)", wb);
    if (tw > DEC_GRID_CAP || tw < wb || (tw - wb) % 2 != 0)
        return fail(ASL_EINVAL, "total_width must be in [width_at_border, %d] and differ from width_at_border by an even number (got %d, width_at_border %d)",
                    DEC_GRID_CAP, tw, wb);
    if (f->ncodes < 1 || f->ncodes > 65535) return fail(ASL_EINVAL, "ncodes must be in [1, 65535] (got %d)", f->ncodes);
    if (!f->bit_x) return fail(ASL_EINVAL, "bit_x is NULL");
    if (!f->bit_y) return fail(ASL_EINVAL, "bit_y is NULL");
    if (!f->codes) return fail(ASL_EINVAL, "codes is NULL");
    std::vector<std::pair<uint64_t, int>> sorted((size_t)f->ncodes);
    for (int i = 0; i < f->ncodes; i++) {
        if (f->codes[i] >> nbits) return fail(ASL_EINVAL, "codes[%d] has bits at or above nbits (%d)", i, nbits);
        sorted[(size_t)i] = {f->codes[i], i};
    }
    std::sort(sorted.begin(), sorted.end());
    for (int i = 1; i < f->ncodes; i++)
        if (sorted[(size_t)i].first == sorted[(size_t)i - 1].first)
            return fail(ASL_EINVAL, "codes[%d] is a duplicate of codes[%d]", sorted[(size_t)i].second, sorted[(size_t)i - 1].second);
    const int off = (tw - wb) / 2;
    int owner[DEC_GRID_CAP * DEC_GRID_CAP];
    for (int &o : owner) o = -1;
    for (int i = 0; i < nbits; i++) {
        const int x = f->bit_x[i], y = f->bit_y[i];
        if (x < -off || y < -off || x >= wb + off || y >= wb + off)
            return fail(ASL_EINVAL, "bit %d at (%d, %d) is outside the total_width grid", i, x, y);
        const bool in_border = x >= 0 && y >= 0 && x < wb && y < wb, in_outer = x >= -1 && y >= -1 && x <= wb && y <= wb;
        if (in_border && (x == 0 || y == 0 || x == wb - 1 || y == wb - 1))
            return fail(ASL_EINVAL, "bit %d at (%d, %d) is on the border ring", i, x, y);
        if (!in_border && in_outer)
            return fail(ASL_EINVAL, "bit %d at (%d, %d) is on the ring just outside the border", i, x, y);
        int &o = owner[(y + off) * tw + (x + off)];
        if (o >= 0) return fail(ASL_EINVAL, "bit %d and bit %d share the cell (%d, %d)", o, i, x, y);
        o = i;
    }
    const int q = nbits / 4;
    for (int i = 0; i + q < 4 * q; i++)
        if (f->bit_x[i + q] != wb - 1 - f->bit_y[i] || f->bit_y[i + q] != f->bit_x[i])
            return fail(ASL_EINVAL, "the layout does not turn with the code: bit %d must be at (%d, %d), the quarter turn of bit %d", i + q,
                        wb - 1 - f->bit_y[i], f->bit_x[i], i);
    if (nbits % 4 == 1 && (wb % 2 == 0 || f->bit_x[nbits - 1] != (wb - 1) / 2 || f->bit_y[nbits - 1] != (wb - 1) / 2))
        return fail(ASL_EINVAL, "the layout does not turn with the code: the last bit must be at the centre cell");
    return ASL_OK;
}

// What a detector of several families assumes on top of asl_family_check of each: global ids id_base[i] + k that fit the
// 16 bits the de-duplication key gives an id (k_dedup.inc) and name one family each.
extern "C" int asl_families_check(const asl_family *fams, const int32_t *id_base, int n_fams)
{
    if (n_fams < 1 || n_fams > ASL_MAX_FAMILIES) return fail(ASL_EINVAL, "n_fams must be in [1, %d] (got %d)", ASL_MAX_FAMILIES, n_fams);
    if (!fams) return fail(ASL_EINVAL, "fams is NULL");
    if (!id_base) return fail(ASL_EINVAL, "id_base is NULL");
    for (int i = 0; i < n_fams; i++) {
        if (asl_family_check(&fams[i])) {
            const std::string why = g_err;
            return fail(ASL_EINVAL, "family %d: %s", i, why.c_str());
        }
        if (id_base[i] < 0) return fail(ASL_EINVAL, "family %d: id_base must not be negative (got %d)", i, (int)id_base[i]);
        const long long end = (long long)id_base[i] + fams[i].ncodes;
        if (end > 65536)
            return fail(ASL_EINVAL, "family %d: id_base + ncodes must not exceed 65536, an id has 16 bits in the de-duplication key (got %d + %d)", i,
                        (int)id_base[i], (int)fams[i].ncodes);
    }
    for (int i = 1; i < n_fams; i++)
        for (int j = 0; j < i; j++)
            if (id_base[i] < id_base[j] + fams[j].ncodes && id_base[j] < id_base[i] + fams[i].ncodes)
                return fail(ASL_EINVAL, "family %d: id_base range [%d, %d) overlaps that of family %d, [%d, %d)", i, (int)id_base[i],
                            (int)(id_base[i] + fams[i].ncodes), j, (int)id_base[j], (int)(id_base[j] + fams[j].ncodes));
    return ASL_OK;
}

static int detector_create(const asl_family *fams, const int32_t *id_base, int n_fams, int default_ids, int maxhamming, float decimate, float blur,
                           int refine_edges, int device, asl_detector **out);

static const asl_family kTag41h12Family = {kTag41h12NBits, kTag41h12WidthAtBorder, kTag41h12TotalWidth, 1, kTag41h12NCodes, 0,
                                           kTag41h12BitX, kTag41h12BitY, reinterpret_cast<const uint64_t *>(kTag41h12Codes)};

extern "C" int asl_detector_create(const char *family, int nthreads, int maxhamming, float decimate, float blur,
                                   int refine_edges, int device, asl_detector **out)
{
    (void)nthreads;  // host threading is meaningless here: the parallelism is the GPU grid
    if (!out) return fail(ASL_EINVAL, "out is NULL");
    *out = nullptr;
    if (!family || strcmp(family, "tagStandard41h12") != 0)
        return fail(ASL_EINVAL, "unknown tag family '%s' (supported: tagStandard41h12)", family ? family : "(null)");
    // ids the reference's own tag images pin; asl_detector_set_id_limit opens the rest
    const int32_t base = 0;
    return detector_create(&kTag41h12Family, &base, 1, kTag41h12PinnedIds, maxhamming, decimate, blur, refine_edges, device, out);
}

extern "C" int asl_detector_create_family(const asl_family *fam, int nthreads, int maxhamming, float decimate, float blur,
                                          int refine_edges, int device, asl_detector **out)
{
    (void)nthreads;
    if (!out) return fail(ASL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = asl_family_check(fam)) return rc;
    const int32_t base = 0;
    return detector_create(fam, &base, 1, 0, maxhamming, decimate, blur, refine_edges, device, out);  // the caller's table: all of its ids
}

extern "C" int asl_detector_create_families(const asl_family *fams, const int32_t *id_base, int n_fams, int nthreads, int maxhamming, float decimate,
                                            float blur, int refine_edges, int device, asl_detector **out)
{
    (void)nthreads;
    if (!out) return fail(ASL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = asl_families_check(fams, id_base, n_fams)) return rc;
    return detector_create(fams, id_base, n_fams, 0, maxhamming, decimate, blur, refine_edges, device, out);
}

// k_decode serves one family whose ids are reported as they are; k_decode_multi every other detector (several families, or
// one made by asl_detector_create_families with an id_base of its own).
static bool decodes_multi(const asl_detector *d) { return d->nfam > 1 || d->fams[0].id_base != 0; }

// The table k_decode_multi reads: the families' device records as they stand (code books and indices included).
static int upload_family_table(asl_detector *d)
{
    if (!decodes_multi(d)) return 0;
    FamilyTabDev tab;
    memset(&tab, 0, sizeof tab);
    tab.n = d->nfam;
    int k = 0;
    for (int i = 0; i < d->nfam; i++) {
        tab.fam[i] = d->fams[i].dev;
        tab.id_base[i] = d->fams[i].id_base;
        bool first = true;  // of its border width
        for (int j = 0; j < i; j++) first = first && d->fams[j].dev.width_at_border != d->fams[i].dev.width_at_border;
        for (int j = i; first && j < d->nfam; j++)
            if (d->fams[j].dev.width_at_border == d->fams[i].dev.width_at_border) tab.order[k++] = j;
    }
    if (d->fam_tab.ensure(1)) return -1;
    return hipMemcpy(d->fam_tab.p, &tab, sizeof tab, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}

// default_ids: the ids a one-family detector decodes until asl_detector_set_id_limit says otherwise; 0: every id of every table
static int detector_create(const asl_family *fams, const int32_t *id_base, int n_fams, int default_ids, int maxhamming, float decimate, float blur,
                           int refine_edges, int device, asl_detector **out)
{
    if (!(decimate >= 1.0f) || decimate != std::floor(decimate) || decimate > 8.0f)
        return fail(ASL_EINVAL, "decimate must be an integer value in [1, 8] (got %g)", (double)decimate);
    if (blur != 0.0f) return fail(ASL_EINVAL, "blur must be 0 here: set quad_sigma with asl_detector_set_quad_sigma");
    if (maxhamming < 0 || maxhamming > 3) return fail(ASL_EINVAL, "maxhamming must be in [0, 3]");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(ASL_EDEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(ASL_EINVAL, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<asl_detector> d(new asl_detector());  // freed with everything it holds on every failure below
    d->device = device;
    d->maxhamming = maxhamming;
    d->decimate = (int)decimate;
    d->refine = refine_edges ? 1 : 0;
    d->nfam = n_fams;
    for (int fi = 0; fi < n_fams; fi++) {
        const asl_family *family = &fams[fi];
        asl_detector::Family &slot = d->fams[fi];
        FamilyDev &f = slot.dev;
        memset(&f, 0, sizeof f);
        f.nbits = family->nbits;
        f.width_at_border = family->width_at_border;
        f.total_width = family->total_width;
        f.reversed_border = family->reversed_border ? 1 : 0;
        f.ncodes = default_ids > 0 ? default_ids : family->ncodes;
        for (int i = 0; i < family->nbits; i++) { f.bit_x[i] = family->bit_x[i]; f.bit_y[i] = family->bit_y[i]; }
        slot.id_base = id_base[fi];
        slot.host_codes.assign(family->codes, family->codes + family->ncodes);
        if (slot.codes.ensure(slot.host_codes.size())) return fail(ASL_ENOMEM, "hipMalloc(code book) failed");
        if (hipMemcpy(slot.codes.p, slot.host_codes.data(), sizeof(unsigned long long) * slot.host_codes.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(ASL_EDEVICE, "hipMemcpy(code book) failed");
        f.codes = slot.codes.p;
        if (build_code_index(d.get(), slot)) return fail(ASL_ENOMEM, "code-book index allocation failed");
    }
    if (upload_family_table(d.get())) return fail(ASL_ENOMEM, "family table allocation failed");
    if (d->wtab.ensure(WEIGHT_TABLE_N)) return fail(ASL_ENOMEM, "hipMalloc(weight table) failed");
    hipLaunchKernelGGL(k_weight_table, dim3((WEIGHT_TABLE_N + 255) / 256), dim3(256), 0, 0, d->wtab.p);
    if (hipDeviceSynchronize() != hipSuccess) return fail(ASL_EDEVICE, "weight table kernel failed");
    // class-3 quad fit uses 64 KB of dynamic LDS on top of a few hundred static bytes
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fit_quads<256, CLASS3_CAP / 256>), hipFuncAttributeMaxDynamicSharedMemorySize, QUAD_LDS_BYTES(CLASS3_CAP));
    *out = d.release();
    return ASL_OK;
}

extern "C" void asl_detector_destroy(asl_detector *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->pending) (void)hipStreamSynchronize(d->p_stream);  // a batch still in flight reads and writes the workspace
    delete d;
}

extern "C" int asl_detector_set_id_limit(asl_detector *d, int n_ids)
{
    if (!d) return fail(ASL_EINVAL, "detector is NULL");
    if (d->nfam > 1) return fail(ASL_EINVAL, "a detector of %d families decodes every id of its tables: the id limit is for one family", d->nfam);
    const int table_ids = (int)d->fams[0].host_codes.size();
    if (n_ids > table_ids) return fail(ASL_EINVAL, "the code table holds %d ids (asked for %d)", table_ids, n_ids);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    d->fams[0].dev.ncodes = n_ids <= 0 ? table_ids : n_ids;
    HIPCHK(hipSetDevice(d->device));
    if (build_code_index(d, d->fams[0]) || upload_family_table(d)) return fail(ASL_ENOMEM, "code-book index allocation failed");
    return ASL_OK;
}

extern "C" int asl_detector_family_of(const asl_detector *d, int id, int *family_index, int *local_id)
{
    if (!d) return fail(ASL_EINVAL, "detector is NULL");
    if (!family_index || !local_id) return fail(ASL_EINVAL, "family_index or local_id is NULL");
    for (int i = 0; i < d->nfam; i++) {
        const int base = d->fams[i].id_base;
        if (id >= base && id - base < (int)d->fams[i].host_codes.size()) {
            *family_index = i; *local_id = id - base;
            return ASL_OK;
        }
    }
    return fail(ASL_EINVAL, "id %d is in no family's range", id);
}

// The taps of tests/blur_ref.py: ksz = int(4 * |sigma|) in float32, made odd; floor(255 * normalised Gaussian) in double.
// Returns ksz (0: off), or -1 for a sigma the detector does not take.
static int blur_kernel(float quad_sigma, uint8_t taps[2 * BLUR_HALO + 1])
{
    if (!std::isfinite(quad_sigma) || !(std::fabs(quad_sigma) < 4.0f)) return -1;
    const float sigma = std::fabs(quad_sigma);
    int ksz = (int)(4.0f * sigma);
    if ((ksz & 1) == 0) ksz++;
    if (ksz <= 1) return 0;
    double dk[2 * BLUR_HALO + 1], sum = 0.0;
    for (int i = 0; i < ksz; i++) {
        const double x = (double)(i - ksz / 2) / (double)sigma;
        dk[i] = std::exp(-0.5 * (x * x));
        sum += dk[i];
    }
    for (int i = 0; i < ksz; i++) taps[i] = (uint8_t)std::floor(dk[i] / sum * 255.0);
    return ksz;
}

extern "C" int asl_blur_taps(float quad_sigma, uint8_t *taps, int max_taps, int *ksz)
{
    if (!ksz) return fail(ASL_EINVAL, "ksz is NULL");
    uint8_t k[2 * BLUR_HALO + 1];
    const int n = blur_kernel(quad_sigma, k);
    if (n < 0) return fail(ASL_EINVAL, "quad_sigma must be finite and |quad_sigma| < 4 (got %g)", (double)quad_sigma);
    if (n > 0 && (!taps || max_taps < n)) return fail(ASL_EINVAL, "taps too small: need %d (got %d)", n, taps ? max_taps : 0);
    for (int i = 0; i < n; i++) taps[i] = k[i];
    *ksz = n;
    return ASL_OK;
}

extern "C" int asl_detector_set_quad_sigma(asl_detector *d, float quad_sigma)
{
    if (!d) return fail(ASL_EINVAL, "detector is NULL");
    uint8_t k[2 * BLUR_HALO + 1];
    const int n = blur_kernel(quad_sigma, k);
    if (n < 0) return fail(ASL_EINVAL, "quad_sigma must be finite and |quad_sigma| < 4 (got %g)", (double)quad_sigma);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    BlurTaps b{};
    b.r = n / 2;  // 0: off
    b.sharpen = quad_sigma < 0.0f ? 1 : 0;
    for (int i = 0; i < n; i++) {  // centred in 15 bytes (k_blur.inc)
        const int u = BLUR_HALO - b.r + i;
        b.k[u >> 2] |= (unsigned int)k[i] << (8 * (u & 3));
    }
    d->blur = b;
    return ASL_OK;
}

extern "C" int asl_detector_set_pnp_both_minima(asl_detector *d, int enabled)
{
    if (!d) return fail(ASL_EINVAL, "detector is NULL");
    d->pnp_both_minima = enabled ? 1 : 0;
    return ASL_OK;
}

extern "C" int asl_set_profiling(asl_detector *d, int enabled)
{
    if (!d) return fail(ASL_EINVAL, "detector is NULL");
    d->profiling = enabled ? 1 : 0;
    if (enabled)
        for (int i = 0; i <= MAX_STAGES; i++)
            if (!d->ev[i]) HIPCHK(hipEventCreate(&d->ev[i]));
    return ASL_OK;
}

extern "C" int asl_stage_times(asl_detector *d, const char **names, float *ms, int max_n, int *n)
{
    if (!d || !n) return fail(ASL_EINVAL, "NULL argument");
    int k = std::min(max_n, d->nstages);
    for (int i = 0; i < k; i++) { if (names) names[i] = d->stage_names[i]; if (ms) ms[i] = d->stage_ms[i]; }
    static const char *hn[4] = {"host_enqueue", "host_wait", "host_copy", "host_post"};
    for (int i = 0; i < 4 && k < max_n; i++, k++) { if (names) names[k] = hn[i]; if (ms) ms[k] = d->host_ms[i]; }
    *n = k;
    return ASL_OK;
}

// Tags per 64-lane wave of the PnP kernels (k_pnp.inc: a quad of lanes per tag, so at most 16): fewer when the launch
// cannot fill the chip anyway, so that a wave is not held up by the slowest of 16 tags.  `expected` = tags in the launch.
static int pnp_tpw(size_t expected)
{
    const char *e = getenv("ASL_PNP_TPW");  // tuning override
    if (e) { int x = atoi(e); return x < 1 ? 1 : (x > 16 ? 16 : x); }
    int v = 1;  // about a wave per SIMD (1024 of them) before the waves fill up: 20 K tags ran 0.153 / 0.193 / 0.256 ms at 16 / 8 / 4 tags per wave
    while (v < 16 && (size_t)v * 2 * 1024 <= expected) v <<= 1;
    return v;
}

static unsigned int next_pow2(unsigned long long v)
{
    unsigned long long p = 1;
    while (p < v) p <<= 1;
    return (unsigned int)p;
}

static int make_geom(asl_detector *d, int n_frames, int channels, int w, int h, int stride, size_t frame_pitch, Geom *g)
{
    if (n_frames <= 0 || n_frames > 65535) return fail(ASL_EINVAL, "n_frames must be in [1, 65535] (got %d)", n_frames);
    if (channels != 1 && channels != 3) return fail(ASL_EINVAL, "channels must be 1 (gray) or 3 (BGR), got %d", channels);
    if (w < 8 || h < 8 || w > 16384 || h > 16384) return fail(ASL_EINVAL, "unsupported image size %dx%d", w, h);
    if (stride < w * channels) return fail(ASL_EINVAL, "stride %d smaller than a row (%d bytes)", stride, w * channels);
    g->w = w; g->h = h; g->stride = stride; g->channels = channels; g->f = d->decimate;
    g->sw = 1 + (w - 1) / g->f; g->sh = 1 + (h - 1) / g->f;
    g->tw = g->sw / TILESZ; g->th = g->sh / TILESZ;
    g->nframes = n_frames; g->frame_pitch = frame_pitch;
    g->npix = (size_t)g->sw * g->sh;
    if (g->npix >= (1u << CLUSTER_LABEL_BITS)) return fail(ASL_EINVAL, "decimated frame has %zu pixels; the cluster key holds 2^24", g->npix);
    return ASL_OK;
}

static int seg_nwx(const Geom &g) { return (g.sw + 63) / 64; }                       // 64-pixel words per row
static int seg_point_tiles_y(const Geom &g) { return std::max(1, (g.sh - 1 + SEG_PH - 1) / SEG_PH); }  // k_seg_points tiles: rows 63k .. 63k+62 emit
static size_t count_tiles(const Geom &g) { return (size_t)seg_nwx(g) * (size_t)seg_point_tiles_y(g); }

static int ensure_workspace(asl_detector *d, const Geom &g)
{
    size_t B = (size_t)g.nframes;
    size_t total = B * g.npix;
    d->nslots = next_pow2(std::max<unsigned long long>(16384ull, (unsigned long long)B * d->hash_slots_per_frame));
    unsigned long long mc = (unsigned long long)B * d->clusters_per_frame;
    d->max_clusters = (unsigned int)std::min<unsigned long long>(mc, 0x7FFFFFFFull);
    unsigned long long mp = (unsigned long long)((double)total * d->points_per_pixel) + 65536ull;
    d->max_points = (unsigned int)std::min<unsigned long long>(mp, 0xFFFFFFF0ull);
    d->max_dets = (unsigned int)std::min<unsigned long long>((unsigned long long)B * d->dets_per_frame, 0x7FFFFFFFull);
    int bad = 0;
    d->qgray = nullptr;  // set by the enqueue; the buffers below may move
    bad |= d->dgray.ensure(total);
    if (d->blur.r) bad |= d->bgray.ensure(total);
    bad |= d->tmin.ensure(B * (size_t)std::max(1, g.tw * g.th) + 8);  // + 8: k_tile_cut's last 8-byte load
    bad |= d->tmax.ensure(B * (size_t)std::max(1, g.tw * g.th) + 8);
    bad |= d->tcut.ensure(B * (size_t)std::max(1, g.tw * g.th));
    bad |= d->parent.ensure(total);
    bad |= d->sizes.ensure(total);
    bad |= d->rootmask.ensure(B * (size_t)g.sh * (size_t)seg_nwx(g));
    bad |= d->wmask.ensure(B * (size_t)g.sh * (size_t)seg_nwx(g));
    bad |= d->bmask.ensure(B * (size_t)g.sh * (size_t)seg_nwx(g));
    bad |= d->hkeys.ensure(d->nslots);
    bad |= d->hcounts.ensure(d->nslots);
    bad |= d->class_lists.ensure((size_t)NCLASSES * d->max_clusters);
    bad |= d->slot_cluster.ensure(d->nslots);
    bad |= d->clusters.ensure(d->max_clusters);
    bad |= d->quads.ensure(d->max_clusters);
    bad |= d->quad_list.ensure(d->max_clusters);
    bad |= d->quadH.ensure((size_t)10 * d->max_clusters);
    bad |= d->side_mom.ensure((size_t)24 * d->max_clusters);
    bad |= d->points.ensure(d->max_points);
    d->stage_cap = (unsigned int)((double)g.npix * d->points_per_pixel) + 1024u;
    bad |= d->stage_rec.ensure((size_t)B * d->stage_cap);
    bad |= d->stage_pos.ensure((size_t)B * d->stage_cap);
    bad |= d->frame_cursor.ensure(B);
    bad |= d->dense_tiles.ensure(B * count_tiles(g));
    bad |= d->dense_seg.ensure(B * (size_t)seg_nwx(g) * (size_t)((g.sh + SEG_TH - 1) / SEG_TH));
    bad |= d->seg_edges.ensure(B * (size_t)seg_nwx(g) * (size_t)((g.sh + SEG_TH - 1) / SEG_TH));
    bad |= d->scratch.ensure((size_t)d->max_points * 8);
    bad |= d->dets.ensure(d->max_dets);
    bad |= d->frame_ndets.ensure(B);
    bad |= d->frame_nkeep.ensure(B);
    bad |= d->frame_off.ensure(B);
    bad |= d->frame_idx.ensure(B * (size_t)d->dets_per_frame);
    bad |= d->out_det.ensure(d->max_dets);
    bad |= d->out_pose.ensure(d->max_dets);
    bad |= d->counters.ensure(CNT__N);
    if (bad) return fail(ASL_ENOMEM, "device workspace allocation failed (%zu frames of %dx%d)", B, g.sw, g.sh);
    return ASL_OK;
}

#define STAGE(name)                                                        \
    do {                                                                   \
        if (d->profiling && d->nev < MAX_STAGES) {                         \
            d->stage_names[d->nev] = name;                                 \
            HIPCHK(hipEventRecord(d->ev[d->nev], st));                     \
            d->nev++;                                                      \
        }                                                                  \
    } while (0)

// S8 (k_dedup.inc): the four launches of the de-duplication over B frames.  enqueue_detect and asl_debug_dedup both come
// through here, so the diagnostic runs the product's launch shapes.  frame_ndets must be zero and counters[CNT_NDETS]
// hold the number of records when the first kernel starts.
struct S8Buffers {
    const DetRec *dets;
    long long *counters;
    unsigned int max_dets;   // records dets holds; out_det / out_pose hold as many
    unsigned int *frame_ndets, *frame_idx;
    unsigned int cap_f;      // entries of frame_idx per frame
    unsigned int *frame_nkeep, *frame_off;
    DetOut *out_det;
    PoseOut *out_pose;       // not written without poses
};
static void launch_dedup(const S8Buffers &b, unsigned int B, int with_pose, hipStream_t st)
{
    hipLaunchKernelGGL(k_det_bucket, dim3((b.max_dets + 255) / 256), dim3(256), 0, st, b.dets, b.counters, b.max_dets, b.frame_ndets, b.frame_idx, b.cap_f,
                       b.counters);
    hipLaunchKernelGGL(k_det_dedup, dim3(B), dim3(256), 0, st, b.dets, b.counters, b.frame_ndets, b.frame_idx, b.cap_f, b.frame_nkeep, b.counters);
    hipLaunchKernelGGL(k_det_offsets, dim3(1), dim3(1024), 0, st, b.frame_nkeep, B, b.frame_off, b.counters);
    hipLaunchKernelGGL(k_det_gather, dim3((b.cap_f + 255) / 256, B), dim3(256), 0, st, b.dets, b.frame_idx, b.cap_f, b.frame_nkeep, b.frame_off, b.out_det,
                       b.out_pose, b.max_dets, with_pose);
}

// tag width in decimated pixels, at least 3 (the quad fit and its finish)
static int tag_width(const asl_detector *d, const Geom &g)
{
    int w = std::max(3, d->fams[0].dev.width_at_border / g.f);
    for (int i = 1; i < d->nfam; i++) w = std::min(w, std::max(3, d->fams[i].dev.width_at_border / g.f));  // upstream: the smallest of the families'
    return w;
}

// which border polarities the families want: bit 0 normal, bit 1 reversed (k_refine's selection, the quad fit's two wants)
static int wanted_polarities(const asl_detector *d)
{
    int m = 0;
    for (int i = 0; i < d->nfam; i++) m |= d->fams[i].dev.reversed_border ? 2 : 1;
    return m;
}

// Quad fit of one size class (k_quad.inc): grid-stride kernels over the class's device-side cluster list -- many more
// workgroups than fit on the chip, so the heavy-tailed per-cluster costs balance out (workgroups without work leave at once).
// CAP: the class's largest cluster, all in LDS; 0 for the global-slab class.
template <int BLOCK, int CAP>
static void launch_fit(asl_detector *d, const Geom &g, int cls, unsigned int grid, hipStream_t st)
{
    const int want_rev = (wanted_polarities(d) >> 1) & 1, want_norm = wanted_polarities(d) & 1;
    hipLaunchKernelGGL((k_fit_quads<BLOCK, CAP / BLOCK>), dim3(grid), dim3(BLOCK), CAP > 0 ? QUAD_LDS_BYTES(CAP) : 0, st, d->clusters.p,
                       d->class_lists.p + (size_t)cls * d->max_clusters, d->counters.p, cls, d->max_clusters, CAP, d->points.p, d->qgray, g,
                       tag_width(d, g), want_rev, want_norm, d->scratch.p, d->quads.p, d->wtab.p, d->side_mom.p);
}

static void launch_fit_class(asl_detector *d, const Geom &g, int cls, unsigned int B, hipStream_t st)
{
    const unsigned int qgrid = std::min<unsigned int>(d->max_clusters, std::max<unsigned int>(16384u, 32u * B));
    const unsigned int q2grid = std::min<unsigned int>(d->max_clusters, 2048u);
    switch (cls) {
    case 0: return launch_fit<64, CLASS0_CAP>(d, g, 0, qgrid, st);
    // two wavefronts per cluster: the 16 KB slab limits a CU to 7 workgroups, so wider workgroups keep more waves in flight
    case 1: return launch_fit<128, CLASS1_CAP>(d, g, 1, qgrid, st);
    case 2: return launch_fit<256, CLASS2_CAP>(d, g, 2, q2grid, st);
    case 3: return launch_fit<256, CLASS3_CAP>(d, g, 3, q2grid, st);
    default: return launch_fit<256, 0>(d, g, 4, q2grid, st);
    }
}

static void launch_quad_finish(asl_detector *d, const Geom &g, hipStream_t st)
{
    hipLaunchKernelGGL(k_quad_finish, dim3(std::min<unsigned int>((d->max_clusters + 63) / 64, 4096u)), dim3(256), 0, st, d->quads.p, d->side_mom.p, d->counters.p,
                       d->max_clusters, tag_width(d, g));
}

// enqueue the whole detector for frames resident at d_frames; no host sync
static int enqueue_detect(asl_detector *d, const uint8_t *d_frames, const Geom &g, hipStream_t st, const CamDev *cam)
{
    dim3 blk(64, 4, 1);
    int thx = (g.sh + TILESZ - 1) / TILESZ;  // generic decimation kernel: tile rows
    unsigned int B = (unsigned int)g.nframes;
    d->nev = 0;
    range_push("S0-S4 gray, decimate, threshold, segmentation, clusters");
    STAGE("k_hash_clear");
    hipLaunchKernelGGL(k_hash_clear, dim3((std::max<unsigned int>(d->nslots, std::max<unsigned int>(B, CNT__N)) + 255) / 256), dim3(256), 0, st, d->hkeys.p,
                       d->hcounts.p, d->nslots, d->counters.p, d->frame_cursor.p, d->frame_ndets.p, B);

    STAGE("k_decimate_minmax");
    if (g.f == 2) {
        const unsigned int ntile = (unsigned int)(g.tw * g.th);
        const unsigned int nrest = (unsigned int)(g.sw - 4 * g.tw) * (unsigned int)g.sh + (unsigned int)(g.sh - 4 * g.th) * (unsigned int)(4 * g.tw);
        if (ntile)
            hipLaunchKernelGGL((g.channels == 1 ? k_decimate2_tiles<1> : k_decimate2_tiles<3>), dim3((ntile + 255) / 256, B), dim3(256), 0, st, d_frames, g,
                               d->dgray.p, d->tmin.p, d->tmax.p);
        if (nrest)
            hipLaunchKernelGGL((g.channels == 1 ? k_decimate_rest<1> : k_decimate_rest<3>), dim3((nrest + 255) / 256, B), dim3(256), 0, st, d_frames, g,
                               d->dgray.p);
    } else
        hipLaunchKernelGGL((g.channels == 1 ? k_decimate_minmax<1> : k_decimate_minmax<3>), dim3((g.sw + 63) / 64, (thx + 3) / 4, B), blk, 0, st, d_frames, g, d->dgray.p, d->tmin.p, d->tmax.p);

    d->qgray = d->dgray.p;
    if (d->blur.r) {  // quad_sigma: the tile cut, the threshold and the quad fit read the blurred image from here on
        STAGE("k_quad_blur");
        hipLaunchKernelGGL(k_quad_blur, dim3((g.sw + BLUR_TW - 1) / BLUR_TW, (g.sh + BLUR_TH - 1) / BLUR_TH, B), dim3(256), 0, st, d->dgray.p, g, d->blur,
                           d->bgray.p, d->tmin.p, d->tmax.p);
        d->qgray = d->bgray.p;
    }

    const int nwx = seg_nwx(g), pty = seg_point_tiles_y(g);
    const size_t nwords = (size_t)B * g.sh * nwx;
    STAGE("k_tile_cut");
    if (g.tw > 0 && g.th > 0)
        hipLaunchKernelGGL(k_tile_cut, dim3((((g.tw + 3) / 4) * ((g.th + 3) / 4) + 255) / 256, B), dim3(256), 0, st, d->tmin.p, d->tmax.p, g, d->tcut.p);
    STAGE("k_seg_tile");
    {
        const int ntiles = nwx * ((g.sh + SEG_TH - 1) / SEG_TH);
        hipLaunchKernelGGL(k_seg_tile, dim3((ntiles + SEG_TILE_WAVES - 1) / SEG_TILE_WAVES, 1, B), dim3(64 * SEG_TILE_WAVES), 0, st, d->qgray, d->tcut.p, g, nwx, ntiles,
                           d->wmask.p, d->bmask.p, d->parent.p, d->sizes.p, d->rootmask.p, d->seg_edges.p, d->dense_seg.p, d->counters.p);
        // tiles with more runs or links than the common launch's tables hold (none in ordinary frames: the launch finds an empty list)
        hipLaunchKernelGGL(k_seg_tile_dense, dim3(1024), dim3(64), 0, st, g, nwx, ntiles, d->wmask.p, d->bmask.p, d->parent.p, d->sizes.p,
                           d->rootmask.p, d->dense_seg.p, d->counters.p);
    }
    STAGE("k_seg_border");
    {
        const size_t nseams = nwx > 1 ? (size_t)B * g.sh * (nwx - 1) : 0;
        const unsigned int ncol_blocks = (unsigned int)((nseams + 63) / 64);
        const int nrb = (g.sh - 1) / SEG_TH;
        const unsigned int nrow_blocks = (unsigned int)nwx * (unsigned int)nrb * (unsigned int)B;
        if (ncol_blocks + nrow_blocks > 0)
            hipLaunchKernelGGL(k_seg_border, dim3(ncol_blocks + nrow_blocks), dim3(64), 0, st, d->wmask.p, d->bmask.p, d->seg_edges.p,
                               nwx * ((g.sh + SEG_TH - 1) / SEG_TH), g, nwx, d->parent.p, d->counters.p, ncol_blocks, nrb > 0 ? nrb : 1);
    }
    STAGE("k_seg_roots");
    hipLaunchKernelGGL(k_seg_roots, dim3((unsigned int)((nwords + 255) / 256)), dim3(256), 0, st, d->rootmask.p, g, nwx, d->parent.p, d->sizes.p);

    STAGE("k_seg_points");
    hipLaunchKernelGGL((k_seg_points<SEGP_PCAP, SEGP_RUNCAP, SEGP_NW, 1>), dim3(B, (nwx + SEGP_NW - 1) / SEGP_NW, pty), dim3(64 * SEGP_NW), 0, st,
                       d->wmask.p, d->bmask.p, g, nwx, d->parent.p, d->sizes.p, d->hkeys.p, d->hcounts.p, d->nslots - 1, d->stage_rec.p,
                       d->stage_pos.p, d->frame_cursor.p, d->stage_cap, d->dense_tiles.p, pty, d->counters.p);
    // tiles of workgroups that ran out of staging space (none in ordinary frames: the launch finds an empty list)
    hipLaunchKernelGGL((k_seg_points<SEGP_PCAP_DENSE, SEGP_RUNCAP_DENSE, 1, 2>), dim3(256), dim3(64), 0, st, d->wmask.p, d->bmask.p, g, nwx,
                       d->parent.p, d->sizes.p, d->hkeys.p, d->hcounts.p, d->nslots - 1, d->stage_rec.p, d->stage_pos.p, d->frame_cursor.p,
                       d->stage_cap, d->dense_tiles.p, pty, d->counters.p);
    STAGE("k_cluster_filter");
    hipLaunchKernelGGL(k_cluster_filter, dim3((d->nslots + 1023) / 1024), dim3(1024), 0, st, d->hkeys.p, d->hcounts.p, d->nslots, g,
                       d->clusters.p, d->slot_cluster.p, d->class_lists.p, d->max_clusters, d->max_points, d->counters.p);
    STAGE("k_point_place");
    hipLaunchKernelGGL(k_point_place, dim3(16, B), dim3(256), 0, st, d->stage_rec.p, d->stage_pos.p, d->frame_cursor.p, d->stage_cap,
                       d->slot_cluster.p, d->points.p, d->counters.p);

    // one launch per size class; each walks its own cluster list (grid-stride)
    range_pop();
    range_push("S5 quad fit");
    for (int cls = 0; cls < NCLASSES; cls++) {
        static const char *const kFitStage[NCLASSES] = {"k_fit_quads<0>", "k_fit_quads<1>", "k_fit_quads<2>", "k_fit_quads<3>", "k_fit_quads<4>"};
        STAGE(kFitStage[cls]);
        launch_fit_class(d, g, cls, B, st);
    }

    STAGE("k_quad_finish");
    launch_quad_finish(d, g, st);
    range_pop();
    range_push("S6-S7 edge refinement, homography, decode");
    STAGE("k_quad_compact");
    hipLaunchKernelGGL(k_quad_compact, dim3((d->max_clusters + 1023) / 1024), dim3(1024), 0, st, d->quads.p, d->counters.p, d->max_clusters,
                       d->quad_list.p);
    unsigned int dgrid = std::min<unsigned int>(d->max_clusters, std::max<unsigned int>(8192u, 64u * B));
    STAGE("k_refine");
    hipLaunchKernelGGL((g.channels == 1 ? k_refine<1> : k_refine<3>), dim3(dgrid), dim3(64), 0, st, d->quads.p, d->counters.p, d->max_clusters, d_frames, g,
                       wanted_polarities(d), d->refine, d->quadH.p, d->quad_list.p, d->side_mom.p);
    STAGE("k_homography");
    hipLaunchKernelGGL(k_homography, dim3(std::min<unsigned int>((d->max_clusters + 31) / 32, 2048u)), dim3(256), 0, st, d->quadH.p, d->counters.p, d->max_clusters,
                       d->quad_list.p, d->side_mom.p);
    STAGE("k_decode");
    if (!decodes_multi(d))
        hipLaunchKernelGGL((g.channels == 1 ? k_decode<1> : k_decode<3>), dim3(dgrid), dim3(64), 0, st, d->quads.p, d->quadH.p, d->counters.p, d->max_clusters, d_frames, g,
                           d->fams[0].dev, d->maxhamming, d->dets.p, d->max_dets, d->counters.p, d->quad_list.p);
    else
        hipLaunchKernelGGL((g.channels == 1 ? k_decode_multi<1> : k_decode_multi<3>), dim3(dgrid), dim3(64), 0, st, d->quads.p, d->quadH.p, d->counters.p, d->max_clusters,
                           d_frames, g, d->fam_tab.p, d->maxhamming, d->dets.p, d->max_dets, d->counters.p, d->quad_list.p);

    range_pop();
    range_push("S9 PnP, S8 de-duplication");
    if (cam) {
        STAGE("k_pnp_dets");
        const int tpw = pnp_tpw(d->nd_guess ? d->nd_guess : (size_t)20 * B);  // detections of the previous batch, else a guess
        hipLaunchKernelGGL(k_pnp_dets, dim3((d->max_dets + tpw - 1) / tpw), dim3(64), 0, st, d->dets.p, d->counters.p, d->max_dets, *cam, tpw);
    }
    // ---- S8: de-duplicate, order by id, lay out the results
    STAGE("k_det_dedup");
    launch_dedup(S8Buffers{d->dets.p, d->counters.p, d->max_dets, d->frame_ndets.p, d->frame_idx.p, d->dets_per_frame, d->frame_nkeep.p, d->frame_off.p,
                           d->out_det.p, d->out_pose.p},
                 B, cam ? 1 : 0, st);
    range_pop();
    if (d->profiling && d->nev <= MAX_STAGES) HIPCHK(hipEventRecord(d->ev[d->nev], st));
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static CamDev make_cam(const asl_detector *d, const double *K, const double *dist, int n_dist, double tag_size)
{
    CamDev c;
    c.both_minima = d->pnp_both_minima; c.pad = 0;
    c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
    c.k1 = c.k2 = c.p1 = c.p2 = c.k3 = 0;
    if (dist && n_dist >= 4) { c.k1 = dist[0]; c.k2 = dist[1]; c.p1 = dist[2]; c.p2 = dist[3]; }
    if (dist && n_dist >= 5) c.k3 = dist[4];
    c.half = (double)(float)(tag_size / 2);  // object corners are float32 in the reference
    return c;
}

using clk = std::chrono::steady_clock;
static float msf(clk::time_point a, clk::time_point b) { return std::chrono::duration<float, std::milli>(b - a).count(); }

// pinned staging of the results: the per-frame counts at the batch's frame count, detections and poses (together) at
// twice what is asked for, 4096 or more
static int ensure_host_out(asl_detector *d, size_t want, size_t nframes)
{
    HIPCHK(d->host_nkeep.ensure(nframes, hipHostMallocDefault));
    if (want <= d->host_cap()) return ASL_OK;
    d->host_det.release(); d->host_pose.release();
    want = std::max<size_t>(want * 2, 4096);
    HIPCHK(d->host_det.ensure(want, hipHostMallocNonCoherent));  // coarse-grained: CPU-cached
    HIPCHK(d->host_pose.ensure(want, hipHostMallocNonCoherent));
    return ASL_OK;
}

// enqueue one batch and the asynchronous read-back of its counters (and of as many detection records as the
// previous batch produced, so that the usual case needs no second copy); returns without waiting
static int submit_batch(asl_detector *d, const uint8_t *d_frames, const Geom &g, hipStream_t st, const CamDev *cam)
{
    if (d->pending) return fail(ASL_EINVAL, "a batch is already in flight on this detector: collect it first");
    int rc = ensure_workspace(d, g);
    if (rc) return rc;
    d->t_submit = clk::now();
    rc = enqueue_detect(d, d_frames, g, st, cam);
    if (rc) return rc;
    HIPCHK(d->pinned_counters.ensure(CNT__N, hipHostMallocDefault));
    HIPCHK(hipMemcpyAsync(d->pinned_counters.p, d->counters.p, sizeof(long long) * CNT__N, hipMemcpyDeviceToHost, st));
    d->prefetched = 0;
    rc = ensure_host_out(d, std::min<size_t>(d->nd_guess, d->max_dets), (size_t)g.nframes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(d->host_nkeep.p, d->frame_nkeep.p, sizeof(unsigned int) * (size_t)g.nframes, hipMemcpyDeviceToHost, st));
    if (d->nd_guess > 0) {  // as many results as the previous batch produced: the usual case needs no second copy
        size_t guess = std::min<size_t>(d->nd_guess, d->max_dets);
        HIPCHK(hipMemcpyAsync(d->host_det.p, d->out_det.p, guess * sizeof(DetOut), hipMemcpyDeviceToHost, st));
        if (cam) HIPCHK(hipMemcpyAsync(d->host_pose.p, d->out_pose.p, guess * sizeof(PoseOut), hipMemcpyDeviceToHost, st));
        d->prefetched = guess;
    }
    d->pending = true;
    d->p_frames = d_frames; d->p_geom = g; d->p_stream = st; d->p_has_cam = cam != nullptr;
    if (cam) d->p_cam = *cam;
    d->t_enqueued = clk::now();
    return ASL_OK;
}

static int collect_batch(asl_detector *d, asl_detection *out, asl_pose *poses, int max_out, int *n_per_frame, int *n_out)
{
    if (!d->pending) return fail(ASL_EINVAL, "no batch in flight on this detector");
    const Geom g = d->p_geom;
    hipStream_t st = d->p_stream;
    const CamDev *cam = d->p_has_cam ? &d->p_cam : nullptr;
    clk::time_point t0 = d->t_submit, t1 = d->t_enqueued, t2 = t1;
    for (int attempt = 0; attempt < 4; attempt++) {
        if (attempt > 0) {  // a work buffer overflowed: grow it and run the batch again, synchronously
            d->pending = false;
            d->nd_guess = 0;
            int rc = submit_batch(d, d->p_frames, g, st, cam);
            if (rc) return rc;
        }
        HIPCHK(hipStreamSynchronize(st));
        t2 = clk::now();
        memcpy(d->last_counters, d->pinned_counters.p, sizeof(long long) * CNT__N);
        d->last = g;
        long long *c = d->last_counters;
        if (c[CNT_UF_GUARD]) {
            d->pending = false;
            return fail(ASL_ECAPACITY, "a union-find loop hit its iteration guard (%lld times): labels of this batch are not trustworthy", c[CNT_UF_GUARD]);
        }
        bool again = false;
        if (c[CNT_OVERFLOW_HASH]) { d->hash_slots_per_frame *= 4; again = true; }
        if (c[CNT_OVERFLOW_CLUSTERS] || c[CNT_NCLUSTERS] > (long long)d->max_clusters) { d->clusters_per_frame *= 4; again = true; }
        if (c[CNT_OVERFLOW_POINTS]) { d->points_per_pixel *= 2; again = true; }
        if (c[CNT_OVERFLOW_DETS]) { d->dets_per_frame *= 4; again = true; }
        if (again) {
            if (attempt == 3) {
                d->pending = false;
                return fail(ASL_ECAPACITY, "work buffers still overflow after growing (hash %lld clusters %lld points %lld dets %lld)",
                            c[CNT_OVERFLOW_HASH], c[CNT_OVERFLOW_CLUSTERS], c[CNT_OVERFLOW_POINTS], c[CNT_OVERFLOW_DETS]);
            }
            continue;
        }
        break;
    }
    d->pending = false;
    if (d->profiling) {
        d->nstages = d->nev;
        for (int i = 0; i < d->nev; i++) HIPCHK(hipEventElapsedTime(&d->stage_ms[i], d->ev[i], d->ev[i + 1]));
    }
    if (d->last_counters[CNT_DEDUP_LIMIT])
        return fail(ASL_ECAPACITY, "%lld frame(s) hold more than %d detections: the de-duplication does not sort that many", d->last_counters[CNT_DEDUP_LIMIT], DEDUP_MAX);
    size_t nd = (size_t)d->last_counters[CNT_NKEEP];
    if (nd > d->max_dets) nd = d->max_dets;
    if (nd > d->prefetched) {
        size_t have = d->prefetched;
        if (nd > d->host_cap()) have = 0;  // the staging buffers are about to be replaced
        int rc = ensure_host_out(d, nd, (size_t)g.nframes);
        if (rc) return rc;
        HIPCHK(hipMemcpy(d->host_det.p + have, d->out_det.p + have, (nd - have) * sizeof(DetOut), hipMemcpyDeviceToHost));
        if (cam) HIPCHK(hipMemcpy(d->host_pose.p + have, d->out_pose.p + have, (nd - have) * sizeof(PoseOut), hipMemcpyDeviceToHost));
    }
    d->nd_guess = nd + nd / 4 + 256;
    clk::time_point t3 = clk::now();
    // the device has de-duplicated, ordered by (frame, id) and laid the results out in the ABI's structs
    static_assert(sizeof(DetOut) == sizeof(asl_detection) && sizeof(PoseOut) == sizeof(asl_pose), "device results are copied verbatim");
    int total = (int)nd;
    int nw = std::min(total, max_out);
    if (out && nw > 0) memcpy(out, d->host_det.p, (size_t)nw * sizeof(asl_detection));
    if (poses && cam && nw > 0) memcpy(poses, d->host_pose.p, (size_t)nw * sizeof(asl_pose));
    if (n_per_frame) for (int f = 0; f < g.nframes; f++) n_per_frame[f] = (int)d->host_nkeep.p[f];
    if (n_out) *n_out = total;
    d->host_ms[0] = msf(t0, t1); d->host_ms[1] = msf(t1, t2); d->host_ms[2] = msf(t2, t3); d->host_ms[3] = msf(t3, clk::now());
    return ASL_OK;
}

// the lens models the PnP and the solvers take: none, (k1, k2, p1, p2) or (k1, k2, p1, p2, k3)
static int check_n_dist(int n_dist)
{
    if (n_dist != 0 && n_dist != 4 && n_dist != 5) return fail(ASL_EINVAL, "n_dist must be 0, 4 or 5");
    return ASL_OK;
}

static int check_device_args(asl_detector *d, const void *d_frames, int n_frames, int channels, int w, int h, int stride, size_t frame_pitch,
                             int n_dist, Geom *g)
{
    if (!d || !d_frames) return fail(ASL_EINVAL, "NULL detector or frames");
    if (int rc = check_n_dist(n_dist)) return rc;
    HIPCHK(hipSetDevice(d->device));
    int rc = make_geom(d, n_frames, channels, w, h, stride, frame_pitch, g);
    if (rc) return rc;
    if (frame_pitch < (size_t)stride * (size_t)h) return fail(ASL_EINVAL, "frame_pitch smaller than one frame");
    return ASL_OK;
}

extern "C" int asl_submit_batch_device(asl_detector *d, const void *d_frames, int n_frames, int channels, int w, int h, int stride,
                                       size_t frame_pitch, void *stream, const double *K, const double *dist, int n_dist, double tag_size)
{
    Geom g;
    int rc = check_device_args(d, d_frames, n_frames, channels, w, h, stride, frame_pitch, n_dist, &g);
    if (rc) return rc;
    CamDev cam;
    if (K) cam = make_cam(d, K, dist, n_dist, tag_size);
    return submit_batch(d, (const uint8_t *)d_frames, g, (hipStream_t)stream, K ? &cam : nullptr);
}

extern "C" int asl_collect_batch(asl_detector *d, asl_detection *out, asl_pose *poses, int max_out, int *n_per_frame, int *n_out)
{
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (max_out < 0 || (max_out > 0 && !out)) return fail(ASL_EINVAL, "out is NULL");
    HIPCHK(hipSetDevice(d->device));
    return collect_batch(d, out, poses, max_out, n_per_frame, n_out);
}

extern "C" int asl_collect_batch_view(asl_detector *d, const asl_detection **out, const asl_pose **poses, const uint32_t **n_per_frame, int *n_out)
{
    if (!d || !out || !n_per_frame || !n_out) return fail(ASL_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(d->device));
    const bool with_poses = d->p_has_cam;
    int rc = collect_batch(d, nullptr, nullptr, 0, nullptr, n_out);  // waits, checks, fills the detector's page-locked result buffers
    if (rc) return rc;
    *out = reinterpret_cast<const asl_detection *>(d->host_det.p);
    if (poses) *poses = with_poses ? reinterpret_cast<const asl_pose *>(d->host_pose.p) : nullptr;
    *n_per_frame = d->host_nkeep.p;
    return ASL_OK;
}

extern "C" int asl_detect_batch_device(asl_detector *d, const void *d_frames, int n_frames, int channels, int w, int h, int stride,
                                       size_t frame_pitch, void *stream, const double *K, const double *dist, int n_dist,
                                       double tag_size, asl_detection *out, asl_pose *poses, int max_out, int *n_per_frame, int *n_out)
{
    if (max_out < 0 || (max_out > 0 && !out)) return fail(ASL_EINVAL, "out is NULL");
    int rc = asl_submit_batch_device(d, d_frames, n_frames, channels, w, h, stride, frame_pitch, stream, K, dist, n_dist, tag_size);
    if (rc) return rc;
    return collect_batch(d, out, poses, max_out, n_per_frame, n_out);
}

// Frames that start in host memory (the reference's callers hand over numpy frames: simulation_engine.py:219,
// video_detection.py:247-258).  All copies are issued up front on a copy stream, one event per chunk of frames; the
// detector works through the chunks on its own stream, each as soon as its frames have landed, so chunk i's kernels run
// under chunk i+1's transfer and the call takes the time of the transfer plus one chunk's kernels (the PCIe link is the
// bound: 2.76 MB per 720p frame against 3.5 us of kernels).  Results are appended chunk by chunk with the frame index
// of the whole call.  A call of fewer than two chunks is one batch, as before.
#define HOST_CHUNK_FRAMES 64
// frames [f0, f1) into the staging buffer; frames that follow each other in host memory (one array, the usual case) go as
// one transfer (a call per 2.76 MB frame costs ~12 us: 6 ms on 512 frames against 25 ms of transfer)
static hipError_t copy_frames(asl_detector *d, const uint8_t *const *frames, int f0, int f1, size_t pitch, hipStream_t st)
{
    int i = f0;
    while (i < f1) {
        int j = i + 1;
        while (j < f1 && frames[j] == frames[j - 1] + pitch) j++;
        hipError_t e = hipMemcpyAsync(d->in.p + (size_t)i * pitch, frames[i], pitch * (size_t)(j - i), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        i = j;
    }
    return hipSuccess;
}

static int detect_host_frames(asl_detector *d, const uint8_t *const *frames, int n_frames, int channels, int w, int h, int stride,
                              const CamDev *cam, asl_detection *out, asl_pose *poses, int max_out, int *n_per_frame, int *n_out)
{
    Geom g;
    const size_t pitch = (size_t)stride * (size_t)h;
    int rc = make_geom(d, n_frames, channels, w, h, stride, pitch, &g);
    if (rc) return rc;
    if (d->in.ensure(pitch * (size_t)n_frames)) return fail(ASL_ENOMEM, "input staging allocation failed");
    for (int i = 0; i < n_frames; i++)
        if (!frames[i]) return fail(ASL_EINVAL, "frames[%d] is NULL", i);
    int chunk = HOST_CHUNK_FRAMES;
    { const char *e = getenv("ASL_HOST_CHUNK"); if (e && atoi(e) > 0) chunk = atoi(e); }  // tuning override
    const int nchunks = n_frames >= 2 * chunk ? (n_frames + chunk - 1) / chunk : 1;
    if (nchunks == 1) {
        HIPCHK(copy_frames(d, frames, 0, n_frames, pitch, nullptr));
        int rcs = submit_batch(d, d->in.p, g, nullptr, cam);
        if (rcs) return rcs;
        return collect_batch(d, out, poses, max_out, n_per_frame, n_out);
    }
    if (!d->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&d->host_stream, hipStreamNonBlocking));
    }
    while ((int)d->copy_done.size() < nchunks) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        d->copy_done.push_back(e);
    }
    HIPCHK(hipStreamSynchronize(nullptr));  // earlier work of this detector on the null stream may still read d->in
    for (int c = 0; c < nchunks; c++) {
        const int f0 = c * chunk, f1 = std::min(n_frames, f0 + chunk);
        HIPCHK(copy_frames(d, frames, f0, f1, pitch, d->copy_stream));
        HIPCHK(hipEventRecord(d->copy_done[c], d->copy_stream));
    }
    int total = 0;
    for (int c = 0; c < nchunks; c++) {
        const int f0 = c * chunk, f1 = std::min(n_frames, f0 + chunk);
        Geom gc = g;
        gc.nframes = f1 - f0;
        HIPCHK(hipStreamWaitEvent(d->host_stream, d->copy_done[c], 0));
        int rcs = submit_batch(d, d->in.p + (size_t)f0 * pitch, gc, d->host_stream, cam);
        if (rcs) { (void)hipStreamSynchronize(d->copy_stream); return rcs; }
        int nc = 0;
        const int room = std::max(0, max_out - total);
        rcs = collect_batch(d, out ? out + std::min(total, max_out) : nullptr, (poses && cam) ? poses + std::min(total, max_out) : nullptr, room,
                            n_per_frame ? n_per_frame + f0 : nullptr, &nc);
        if (rcs) { (void)hipStreamSynchronize(d->copy_stream); return rcs; }
        for (int k = total; k < std::min(total + nc, max_out); k++) out[k].frame += f0;  // frame index inside the whole call
        total += nc;
    }
    if (n_out) *n_out = total;
    return ASL_OK;
}

extern "C" int asl_detect_batch_u8(asl_detector *d, const uint8_t *const *frames, int n_frames, int channels, int w, int h, int stride,
                                   asl_detection *out, int max_out, int *n_per_frame, int *n_out)
{
    if (!d || !frames) return fail(ASL_EINVAL, "NULL detector or frames");
    if (max_out < 0 || (max_out > 0 && !out)) return fail(ASL_EINVAL, "out is NULL");
    HIPCHK(hipSetDevice(d->device));
    return detect_host_frames(d, frames, n_frames, channels, w, h, stride, nullptr, out, nullptr, max_out, n_per_frame, n_out);
}

extern "C" int asl_detect_batch_pose_u8(asl_detector *d, const uint8_t *const *frames, int n_frames, int channels, int w, int h, int stride,
                                        const double *K, const double *dist, int n_dist, double tag_size, asl_detection *out, asl_pose *poses,
                                        int max_out, int *n_per_frame, int *n_out)
{
    if (!d || !frames || !K || !poses) return fail(ASL_EINVAL, "NULL detector, frames, K or poses");
    if (max_out < 0 || (max_out > 0 && !out)) return fail(ASL_EINVAL, "out is NULL");
    if (int rc = check_n_dist(n_dist)) return rc;
    if (n_dist && !dist) return fail(ASL_EINVAL, "dist is NULL but n_dist = %d", n_dist);
    HIPCHK(hipSetDevice(d->device));
    CamDev cam = make_cam(d, K, dist, n_dist, tag_size);
    return detect_host_frames(d, frames, n_frames, channels, w, h, stride, &cam, out, poses, max_out, n_per_frame, n_out);
}

extern "C" int asl_detect_gray_u8(asl_detector *d, const uint8_t *gray, int w, int h, int stride, asl_detection *out, int max_out, int *n_out)
{
    const uint8_t *fr[1] = {gray};
    return asl_detect_batch_u8(d, fr, 1, 1, w, h, stride, out, max_out, nullptr, n_out);
}

extern "C" int asl_detect_bgr_u8(asl_detector *d, const uint8_t *bgr, int w, int h, int stride, asl_detection *out, int max_out, int *n_out)
{
    const uint8_t *fr[1] = {bgr};
    return asl_detect_batch_u8(d, fr, 1, 3, w, h, stride, out, max_out, nullptr, n_out);
}

extern "C" int asl_render_frames_device(asl_detector *d, void *d_frames, int n_frames, int w, int h, int stride, size_t frame_pitch,
                                        const void *d_planes, int max_planes, const void *d_textures, int tw, int th, double half,
                                        const double *K, const double *dist, int n_dist, void *stream)
{
    if (!d || !d_frames || !d_planes || !d_textures) return fail(ASL_EINVAL, "NULL argument");
    if (n_frames <= 0 || w <= 0 || h <= 0 || max_planes <= 0 || tw <= 0 || th <= 0) return fail(ASL_EINVAL, "sizes must be positive");
    if (stride < 3 * w || frame_pitch < (size_t)stride * (size_t)h) return fail(ASL_EINVAL, "stride / frame_pitch smaller than a BGR row / frame");
    if (dist && n_dist != 4 && n_dist != 5) return fail(ASL_EINVAL, "n_dist must be 4 or 5");
    if (dist && !K) return fail(ASL_EINVAL, "lens coefficients need the camera matrix");
    static_assert(sizeof(RenderPlane) == sizeof(asl_render_plane) && sizeof(asl_render_plane) == 96, "asl_render_plane layout");
    HIPCHK(hipSetDevice(d->device));
    RenderCam cam;
    memset(&cam, 0, sizeof cam);
    cam.iters = 8;
    if (K && dist) {
        cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];
        cam.k1 = dist[0]; cam.k2 = dist[1]; cam.p1 = dist[2]; cam.p2 = dist[3]; cam.k3 = n_dist >= 5 ? dist[4] : 0.0;
        cam.distort = 1;
    }
    hipLaunchKernelGGL(k_render, dim3((w + RENDER_TW - 1) / RENDER_TW, (h + 4 * RENDER_TH - 1) / (4 * RENDER_TH), (unsigned int)n_frames), dim3(64, 4), 0, (hipStream_t)stream, (uint8_t *)d_frames, w, h,
                       stride, frame_pitch, (const RenderPlane *)d_planes, max_planes, (const uint8_t *)d_textures, tw, th, half, cam);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

// ---- lens rectification ahead of the detector (k_rectify.inc).  The detector supplies the device and, for the host form,
// the staging buffers; no batch state is read or written, so both calls are legal while a batch is pending.
struct RectifyCall {
    const void *src; int n_frames, channels, w, h, stride; size_t frame_pitch;
    void *dst; int w_out, h_out, stride_out; size_t frame_pitch_out;
    const double *K, *dist; int n_dist; const double *K_new; int fill;
    int n_views = 1;  // asl_rectify_views_*: the destination holds n_views * n_frames frames
};
#define RECTIFY_MAX_DIM 16384  // the detector's own limit (make_geom); keeps every row offset and the launch grid in range

// every argument check of the two entry points: nothing is written before it passes.  `device`: the frame pitches count.
static int check_rectify_call(const asl_detector *d, const RectifyCall &c, bool device, RectifyCam *cam)
{
    if (!d || !c.src || !c.dst || !c.K) return fail(ASL_EINVAL, "NULL detector, source, destination or K");
    if (c.channels != 1 && c.channels != 3) return fail(ASL_EINVAL, "channels must be 1 (gray) or 3 (BGR), got %d", c.channels);
    if (c.n_frames <= 0 || c.w <= 0 || c.h <= 0 || c.w_out <= 0 || c.h_out <= 0)
        return fail(ASL_EINVAL, "sizes must be positive (n_frames %d, source %dx%d, output %dx%d)", c.n_frames, c.w, c.h, c.w_out, c.h_out);
    if (c.w > RECTIFY_MAX_DIM || c.h > RECTIFY_MAX_DIM || c.w_out > RECTIFY_MAX_DIM || c.h_out > RECTIFY_MAX_DIM)
        return fail(ASL_EINVAL, "unsupported image size (source %dx%d, output %dx%d; at most %d each way)", c.w, c.h, c.w_out, c.h_out, RECTIFY_MAX_DIM);
    if (c.stride < c.w * c.channels) return fail(ASL_EINVAL, "stride %d smaller than a source row (%d bytes)", c.stride, c.w * c.channels);
    if (c.stride_out < c.w_out) return fail(ASL_EINVAL, "stride_out %d smaller than an output row (%d bytes)", c.stride_out, c.w_out);
    if (device && c.frame_pitch < (size_t)c.stride * (size_t)c.h) return fail(ASL_EINVAL, "frame_pitch smaller than one source frame");
    if (device && c.frame_pitch_out < (size_t)c.stride_out * (size_t)c.h_out) return fail(ASL_EINVAL, "frame_pitch_out smaller than one output frame");
    if (int rc = check_n_dist(c.n_dist)) return rc;
    if (c.n_dist && !c.dist) return fail(ASL_EINVAL, "dist is NULL with n_dist = %d", c.n_dist);
    if (c.fill < 0 || c.fill > 255) return fail(ASL_EINVAL, "fill must be in [0, 255] (got %d)", c.fill);
    const double *Kn = c.K_new ? c.K_new : c.K;
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(c.K[k]) || !std::isfinite(Kn[k])) return fail(ASL_EINVAL, "K / K_new is not finite");
    for (int k = 0; k < c.n_dist; k++)
        if (!std::isfinite(c.dist[k])) return fail(ASL_EINVAL, "dist is not finite");
    if (!(c.K[0] > 0) || !(c.K[4] > 0) || !(Kn[0] > 0) || !(Kn[4] > 0)) return fail(ASL_EINVAL, "K and K_new must have positive focal lengths");
    // the bytes the kernel may read / write: whole strides but for the last row of the last frame
    const size_t src_bytes = (size_t)(c.n_frames - 1) * c.frame_pitch + (size_t)(c.h - 1) * (size_t)c.stride + (size_t)c.w * (size_t)c.channels;
    const size_t dst_bytes = ((size_t)c.n_views * (size_t)c.n_frames - 1) * c.frame_pitch_out + (size_t)(c.h_out - 1) * (size_t)c.stride_out + (size_t)c.w_out;
    const uintptr_t s0 = (uintptr_t)c.src, d0 = (uintptr_t)c.dst;
    if (s0 < d0 + dst_bytes && d0 < s0 + src_bytes) return fail(ASL_EINVAL, "source and destination overlap");
    memset(cam, 0, sizeof *cam);
    cam->fx = c.K[0]; cam->fy = c.K[4]; cam->cx = c.K[2]; cam->cy = c.K[5];
    if (c.n_dist) { cam->k1 = c.dist[0]; cam->k2 = c.dist[1]; cam->p1 = c.dist[2]; cam->p2 = c.dist[3]; cam->k3 = c.n_dist >= 5 ? c.dist[4] : 0.0; }
    cam->nfx = Kn[0]; cam->nfy = Kn[4]; cam->ncx = Kn[2]; cam->ncy = Kn[5];
    cam->fill = c.fill;
    return ASL_OK;
}

// frames along blockIdx.z, as many to a launch as the grid takes
static int launch_rectify(const RectifyCall &c, const RectifyCam &cam, hipStream_t st)
{
    const dim3 tiles((c.w_out + RECTIFY_TW - 1) / RECTIFY_TW, (c.h_out + 4 * RECTIFY_TH - 1) / (4 * RECTIFY_TH));
    const unsigned long long per_frame = 256ull * tiles.x * tiles.y;
    const int step = (int)std::max<unsigned long long>(1ull, std::min<unsigned long long>(65535ull, (1ull << 31) / per_frame));
    for (int f0 = 0; f0 < c.n_frames; f0 += step) {
        const dim3 grid(tiles.x, tiles.y, (unsigned int)std::min(step, c.n_frames - f0));
        const uint8_t *s = (const uint8_t *)c.src + (size_t)f0 * c.frame_pitch;
        uint8_t *o = (uint8_t *)c.dst + (size_t)f0 * c.frame_pitch_out;
        if (c.channels == 1)
            hipLaunchKernelGGL(k_rectify<1>, grid, dim3(64, 4), 0, st, s, c.w, c.h, c.stride, c.frame_pitch, o, c.w_out, c.h_out, c.stride_out, c.frame_pitch_out, cam);
        else
            hipLaunchKernelGGL(k_rectify<3>, grid, dim3(64, 4), 0, st, s, c.w, c.h, c.stride, c.frame_pitch, o, c.w_out, c.h_out, c.stride_out, c.frame_pitch_out, cam);
        HIPCHK(hipGetLastError());
    }
    return ASL_OK;
}

extern "C" int asl_rectify_frames_device(asl_detector *d, const void *d_src, int n_frames, int channels, int w, int h, int stride, size_t frame_pitch,
                                         void *d_dst, int w_out, int h_out, int stride_out, size_t frame_pitch_out, const double *K,
                                         const double *dist, int n_dist, const double *K_new, int fill, void *stream)
{
    const RectifyCall c{d_src, n_frames, channels, w, h, stride, frame_pitch, d_dst, w_out, h_out, stride_out, frame_pitch_out, K, dist, n_dist, K_new, fill};
    RectifyCam cam;
    if (int rc = check_rectify_call(d, c, true, &cam)) return rc;
    HIPCHK(hipSetDevice(d->device));
    return launch_rectify(c, cam, (hipStream_t)stream);
}

extern "C" int asl_rectify_u8(asl_detector *d, const uint8_t *src, int channels, int w, int h, int stride, uint8_t *dst, int w_out, int h_out,
                              int stride_out, const double *K, const double *dist, int n_dist, const double *K_new, int fill)
{
    RectifyCall c{src, 1, channels, w, h, stride, 0, dst, w_out, h_out, stride_out, 0, K, dist, n_dist, K_new, fill};
    RectifyCam cam;
    if (int rc = check_rectify_call(d, c, false, &cam)) return rc;
    HIPCHK(hipSetDevice(d->device));
    const size_t row = (size_t)w * (size_t)channels;
    if (d->rect_src.ensure(row * (size_t)h) || d->rect_dst.ensure((size_t)w_out * (size_t)h_out)) return fail(ASL_ENOMEM, "rectification staging allocation failed");
    // rows packed on the device; the padding of the caller's rows is neither read nor written
    HIPCHK(hipMemcpy2D(d->rect_src.p, row, src, (size_t)stride, row, (size_t)h, hipMemcpyHostToDevice));
    c.src = d->rect_src.p; c.stride = (int)row; c.frame_pitch = row * (size_t)h;
    c.dst = d->rect_dst.p; c.stride_out = w_out; c.frame_pitch_out = (size_t)w_out * (size_t)h_out;
    if (int rc = launch_rectify(c, cam, nullptr)) return rc;
    HIPCHK(hipMemcpy2D(dst, (size_t)stride_out, d->rect_dst.p, (size_t)w_out, (size_t)w_out, (size_t)h_out, hipMemcpyDeviceToHost));
    return ASL_OK;
}

// ---- rectification into rotated pinhole views (k_rectify_views): check_rectify_call's checks and those of the lens
// model, the view table and theta_max; the same staging buffers, so both calls are legal while a batch is pending.
#define RECTIFY_ROTATION_TOL 1e-6  // rig.ORTHONORMAL_TOL
static int check_rectify_views_call(const asl_detector *d, const RectifyCall &c, bool device, int lens_model, const asl_rectify_view *views,
                                    double theta_max, RectifyLens *lens, RectifyViewTable *table)
{
    static_assert(sizeof(asl_rectify_view) == 144, "asl_rectify_view layout");
    static_assert(RECTIFY_MAX_VIEWS == ASL_MAX_VIEWS && RECTIFY_LENS_BROWN == ASL_LENS_BROWN && RECTIFY_LENS_FISHEYE == ASL_LENS_FISHEYE, "header and kernel agree");
    if (lens_model != ASL_LENS_BROWN && lens_model != ASL_LENS_FISHEYE) return fail(ASL_EINVAL, "lens_model must be ASL_LENS_BROWN (0) or ASL_LENS_FISHEYE (1), got %d", lens_model);
    if (lens_model == ASL_LENS_FISHEYE && c.n_dist != 0 && c.n_dist != 4) return fail(ASL_EINVAL, "a fisheye lens has n_dist 0 or 4 (k1 k2 k3 k4), got %d", c.n_dist);
    if (c.n_views < 1 || c.n_views > ASL_MAX_VIEWS) return fail(ASL_EINVAL, "n_views must be in 1..%d, got %d", ASL_MAX_VIEWS, c.n_views);
    if (!views) return fail(ASL_EINVAL, "views is NULL");
    if (!device && c.frame_pitch_out < (size_t)std::max(c.stride_out, 0) * (size_t)std::max(c.h_out, 0)) return fail(ASL_EINVAL, "view_pitch_out smaller than one output frame");
    RectifyCam cam;
    if (int rc = check_rectify_call(d, c, device, &cam)) return rc;
    if (!std::isfinite(theta_max) || theta_max < 0 || theta_max > M_PI) return fail(ASL_EINVAL, "theta_max must be 0 (= pi) or in (0, pi]");
    for (int v = 0; v < c.n_views; v++) {
        const double *K = views[v].K, *R = views[v].R;
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(K[k]) || !std::isfinite(R[k])) return fail(ASL_EINVAL, "view %d: K / R is not finite", v);
        if (!(K[0] > 0) || !(K[4] > 0)) return fail(ASL_EINVAL, "view %d: K must have positive focal lengths", v);
        double worst = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                worst = std::max(worst, std::fabs(R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0)));
        const double det3 = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (worst > RECTIFY_ROTATION_TOL || !(det3 > 0)) return fail(ASL_EINVAL, "view %d: R is not a rotation", v);
    }
    memset(lens, 0, sizeof *lens);
    memset(table, 0, sizeof *table);
    lens->fx = c.K[0]; lens->fy = c.K[4]; lens->cx = c.K[2]; lens->cy = c.K[5];
    for (int k = 0; k < c.n_dist; k++) lens->k[k] = c.dist[k];
    lens->theta_max = theta_max == 0 ? M_PI : theta_max;
    lens->fill = c.fill;
    for (int v = 0; v < c.n_views; v++) {
        RectifyView &o = table->v[v];
        o.nfx = views[v].K[0]; o.nfy = views[v].K[4]; o.ncx = views[v].K[2]; o.ncy = views[v].K[5];
        memcpy(o.R, views[v].R, sizeof o.R);
    }
    return ASL_OK;
}

template <int CH, int MODEL>
static void launch_rectify_views_as(const RectifyCall &c, const dim3 &grid, int z0, const RectifyLens &lens, const RectifyViewTable &table, hipStream_t st)
{
    hipLaunchKernelGGL((k_rectify_views<CH, MODEL>), grid, dim3(64, 4), 0, st, (const uint8_t *)c.src, c.n_frames, c.w, c.h, c.stride, c.frame_pitch,
                       (uint8_t *)c.dst, c.w_out, c.h_out, c.stride_out, c.frame_pitch_out, z0, lens, table);
}

// view * n_frames + frame along blockIdx.z, as many to a launch as the grid takes
static int launch_rectify_views(const RectifyCall &c, int lens_model, const RectifyLens &lens, const RectifyViewTable &table, hipStream_t st)
{
    const dim3 tiles((c.w_out + RECTIFY_TW - 1) / RECTIFY_TW, (c.h_out + 4 * RECTIFY_TH - 1) / (4 * RECTIFY_TH));
    const unsigned long long per_frame = 256ull * tiles.x * tiles.y;
    const long long total = (long long)c.n_views * c.n_frames;
    const long long step = (long long)std::max<unsigned long long>(1ull, std::min<unsigned long long>(65535ull, (1ull << 31) / per_frame));
    if (total > 0x7fffffffLL) return fail(ASL_EINVAL, "n_views * n_frames does not fit");
    for (long long z0 = 0; z0 < total; z0 += step) {
        const dim3 grid(tiles.x, tiles.y, (unsigned int)std::min(step, total - z0));
        const bool fish = lens_model == ASL_LENS_FISHEYE;
        if (c.channels == 1 && !fish) launch_rectify_views_as<1, RECTIFY_LENS_BROWN>(c, grid, (int)z0, lens, table, st);
        else if (c.channels == 1) launch_rectify_views_as<1, RECTIFY_LENS_FISHEYE>(c, grid, (int)z0, lens, table, st);
        else if (!fish) launch_rectify_views_as<3, RECTIFY_LENS_BROWN>(c, grid, (int)z0, lens, table, st);
        else launch_rectify_views_as<3, RECTIFY_LENS_FISHEYE>(c, grid, (int)z0, lens, table, st);
        HIPCHK(hipGetLastError());
    }
    return ASL_OK;
}

extern "C" int asl_rectify_views_device(asl_detector *d, const void *d_src, int n_frames, int channels, int w, int h, int stride, size_t frame_pitch,
                                        void *d_dst, int w_out, int h_out, int stride_out, size_t frame_pitch_out, const double *K, const double *dist,
                                        int n_dist, int lens_model, const asl_rectify_view *views, int n_views, double theta_max, int fill, void *stream)
{
    const RectifyCall c{d_src, n_frames, channels, w, h, stride, frame_pitch, d_dst, w_out, h_out, stride_out, frame_pitch_out, K, dist, n_dist, nullptr, fill, n_views};
    RectifyLens lens;
    RectifyViewTable table;
    if (int rc = check_rectify_views_call(d, c, true, lens_model, views, theta_max, &lens, &table)) return rc;
    HIPCHK(hipSetDevice(d->device));
    return launch_rectify_views(c, lens_model, lens, table, (hipStream_t)stream);
}

extern "C" int asl_rectify_views_u8(asl_detector *d, const uint8_t *src, int channels, int w, int h, int stride, uint8_t *dst, int w_out, int h_out,
                                    int stride_out, size_t view_pitch_out, const double *K, const double *dist, int n_dist, int lens_model,
                                    const asl_rectify_view *views, int n_views, double theta_max, int fill)
{
    RectifyCall c{src, 1, channels, w, h, stride, 0, dst, w_out, h_out, stride_out, view_pitch_out, K, dist, n_dist, nullptr, fill, n_views};
    RectifyLens lens;
    RectifyViewTable table;
    if (int rc = check_rectify_views_call(d, c, false, lens_model, views, theta_max, &lens, &table)) return rc;
    HIPCHK(hipSetDevice(d->device));
    const size_t row = (size_t)w * (size_t)channels, view_bytes = (size_t)w_out * (size_t)h_out;
    if (d->rect_src.ensure(row * (size_t)h) || d->rect_dst.ensure(view_bytes * (size_t)n_views)) return fail(ASL_ENOMEM, "rectification staging allocation failed");
    // rows packed on the device; the padding of the caller's rows and views is neither read nor written
    HIPCHK(hipMemcpy2D(d->rect_src.p, row, src, (size_t)stride, row, (size_t)h, hipMemcpyHostToDevice));
    c.src = d->rect_src.p; c.stride = (int)row; c.frame_pitch = row * (size_t)h;
    c.dst = d->rect_dst.p; c.stride_out = w_out; c.frame_pitch_out = view_bytes;
    if (int rc = launch_rectify_views(c, lens_model, lens, table, nullptr)) return rc;
    for (int v = 0; v < n_views; v++)
        HIPCHK(hipMemcpy2D(dst + (size_t)v * view_pitch_out, (size_t)stride_out, d->rect_dst.p + (size_t)v * view_bytes, (size_t)w_out, (size_t)w_out, (size_t)h_out, hipMemcpyDeviceToHost));
    return ASL_OK;
}

extern "C" int asl_pack_observations_device(asl_detector *d, void *d_obs, int max_tags, void *stream)
{
    if (!d || !d_obs) return fail(ASL_EINVAL, "NULL detector or output");
    if (max_tags <= 0) return fail(ASL_EINVAL, "max_tags must be positive");
    if (!d->pending) return fail(ASL_EINVAL, "no batch in flight on this detector: pack between submit and the next submit");
    static_assert(sizeof(ObsRec) == sizeof(asl_obs) && sizeof(asl_obs) == 136, "asl_obs layout");
    HIPCHK(hipSetDevice(d->device));
    const int nf = d->p_geom.nframes;
    const unsigned int total = (unsigned int)nf * (unsigned int)max_tags;
    hipLaunchKernelGGL(k_obs_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, d->dets.p, d->frame_idx.p, d->dets_per_frame,
                       d->frame_nkeep.p, d->counters.p, (ObsRec *)d_obs, nf, max_tags);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_graph_frames_device(asl_detector *d, const void *d_obs, int world, int n_frames, int max_tags, int coordinate_id,
                                       double *d_pose, uint8_t *d_status, uint32_t *d_last, int n_ids, void *d_picks, void *stream)
{
    if (!d || !d_obs || !d_pose || !d_status || !d_last) return fail(ASL_EINVAL, "NULL argument");
    if (world <= 0 || n_frames <= 0 || max_tags <= 0 || n_ids <= 0) return fail(ASL_EINVAL, "sizes must be positive");
    HIPCHK(hipSetDevice(d->device));
    const unsigned int total = (unsigned int)world * (unsigned int)n_frames;
    const int lds_ids = (size_t)n_ids * sizeof(unsigned int) <= 48 * 1024 ? n_ids : 0;  // the table as an LDS copy per workgroup, if it fits
    hipLaunchKernelGGL(k_graph_frames, dim3((total + 255) / 256), dim3(256), sizeof(unsigned int) * (size_t)lds_ids, (hipStream_t)stream, (const ObsRec *)d_obs,
                       world, n_frames, max_tags, coordinate_id, d_pose, d_status, (unsigned int *)d_last, n_ids, lds_ids);
    if (d_picks)
        hipLaunchKernelGGL(k_graph_pick, dim3((n_ids + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const ObsRec *)d_obs, world, n_frames, max_tags,
                           (const unsigned int *)d_last, n_ids, (ObsRec *)d_picks);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_graph_picks_device(asl_detector *d, const void *d_obs, int world, int n_frames, int max_tags, const uint8_t *d_status,
                                      unsigned int order_lo, unsigned int order_hi, uint32_t *d_last, int n_ids, void *d_picks, void *stream)
{
    if (!d || !d_obs || !d_status || !d_last || !d_picks) return fail(ASL_EINVAL, "NULL argument");
    if (world <= 0 || n_frames <= 0 || max_tags <= 0 || n_ids <= 0) return fail(ASL_EINVAL, "sizes must be positive");
    if (order_lo > order_hi) return fail(ASL_EINVAL, "empty or reversed range");
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemsetAsync(d_last, 0, sizeof(uint32_t) * (size_t)n_ids, (hipStream_t)stream));
    const unsigned int total = (unsigned int)world * (unsigned int)n_frames;
    const int lds_ids = (size_t)n_ids * sizeof(unsigned int) <= 48 * 1024 ? n_ids : 0;
    hipLaunchKernelGGL(k_graph_last_range, dim3((total + 255) / 256), dim3(256), sizeof(unsigned int) * (size_t)lds_ids, (hipStream_t)stream, (const ObsRec *)d_obs,
                       world, n_frames, max_tags, d_status, order_lo, order_hi, (unsigned int *)d_last, n_ids, lds_ids);
    hipLaunchKernelGGL(k_graph_pick, dim3((n_ids + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const ObsRec *)d_obs, world, n_frames, max_tags,
                       (const unsigned int *)d_last, n_ids, (ObsRec *)d_picks);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_solve_pnp_batch(asl_detector *d, const float *corners, const double *K, const double *dist, int n_dist,
                                   double tag_size, double *rvec, double *tvec, double *T, uint8_t *ok, int N)
{
    if (!d || !corners || !K || !rvec || !tvec || !T || !ok) return fail(ASL_EINVAL, "NULL argument");
    if (N < 0) return fail(ASL_EINVAL, "N < 0");
    if (int rc = check_n_dist(n_dist)) return rc;
    if (N == 0) return ASL_OK;
    HIPCHK(hipSetDevice(d->device));
    if (d->pnp_corners.ensure((size_t)N * 8) || d->pnp_out.ensure((size_t)N * 22) || d->pnp_ok.ensure((size_t)N))
        return fail(ASL_ENOMEM, "PnP workspace allocation failed");
    CamDev cam = make_cam(d, K, dist, n_dist, tag_size);
    HIPCHK(hipMemcpy(d->pnp_corners.p, corners, sizeof(float) * 8 * (size_t)N, hipMemcpyHostToDevice));
    double *dr = d->pnp_out.p, *dt = dr + 3 * (size_t)N, *dT = dt + 3 * (size_t)N;
    hipLaunchKernelGGL(k_pnp_batch, dim3((N + pnp_tpw((size_t)N) - 1) / pnp_tpw((size_t)N)), dim3(64), 0, nullptr, d->pnp_corners.p, N, cam, dr, dt, dT, d->pnp_ok.p, pnp_tpw((size_t)N));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(rvec, dr, sizeof(double) * 3 * (size_t)N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tvec, dt, sizeof(double) * 3 * (size_t)N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(T, dT, sizeof(double) * 16 * (size_t)N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ok, d->pnp_ok.p, (size_t)N, hipMemcpyDeviceToHost));
    return ASL_OK;
}

#include "gn_host.inc"
#include "solve_host.inc"
#include "debug_host.inc"
