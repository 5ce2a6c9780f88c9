// Host side of the diagnostics (device side: k_seg_debug_* in k_seg.inc, k_div_check below): asl_debug_fetch, the quad-fit
// refit, the de-duplication of given records, the pose-graph back-end's factorisation and single step, the division check
// and the phase counters; each checks the room it may write into before it writes anything.

// asl_debug_division_check: div_by(a, recip_of(d)) (asl_common.h) against a / d, as compiled into this library: log-uniform
// magnitudes with exponents within +-lim, both signs, a = 0 now and then
__global__ void __launch_bounds__(256) k_div_check(unsigned long long seed, int per_thread, int lim, unsigned long long *bad)
{
    unsigned long long s = seed + 0x9E3779B97F4A7C15ull * (blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x + 1);
    auto rng = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int i = 0; i < 8; i++) rng();
    unsigned long long nbad = 0;
    for (int i = 0; i < per_thread; i++) {
        const unsigned long long u = rng(), v = rng(), w = rng();
        const int ea = (int)(u % (unsigned)(2 * lim + 1)) - lim, ed = (int)((u >> 20) % (unsigned)(2 * lim + 1)) - lim;
        double a = ldexp(1.0 + (double)(v & 0xFFFFFFFFFFFFFull) * 0x1p-52, ea);
        double dd = ldexp(1.0 + (double)(w & 0xFFFFFFFFFFFFFull) * 0x1p-52, ed);
        if (u & (1ull << 60)) a = -a;
        if (u & (1ull << 61)) dd = -dd;
        if ((u >> 40) % 257 == 0) a = 0.0;
        const double want = a / dd, got = div_by(a, recip_of(dd));
        if (__double_as_longlong(want) != __double_as_longlong(got)) nbad++;
    }
    if (nbad) atomicAdd(bad, nbad);
}

// asl_debug_fetch items 1 and 3: the last batch's threshold image as bytes, into d->dbg_thresh (the pipeline keeps it as
// two bit masks per 64 pixels)
static int expand_thresh(asl_detector *d, const Geom &g, size_t total)
{
    if (d->dbg_thresh.ensure(total)) return fail(ASL_ENOMEM, "debug buffer allocation failed");
    hipLaunchKernelGGL(k_seg_debug_thresh, dim3((g.sw + 63) / 64, (g.sh + 3) / 4, (unsigned int)g.nframes), dim3(64, 4), 0, nullptr,
                       d->wmask.p, d->bmask.p, g, seg_nwx(g), d->dbg_thresh.p);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_debug_fetch(asl_detector *d, int what, void *dst, size_t bytes, size_t *n_items)
{
    if (!d || !dst || !n_items) return fail(ASL_EINVAL, "NULL argument");
    HIPCHK(hipSetDevice(d->device));
    const Geom &g = d->last;
    size_t total = (size_t)g.nframes * g.npix;
    if (((what >= 0 && what <= 3) || what == 9) && total == 0) return fail(ASL_EINVAL, "no batch has run yet");
    switch (what) {
    case 0:    // the image the threshold read: k_quad_blur's under quad_sigma
    case 9: {  // the decimation's own output (7 and 8 are retired numbers and stay unknown)
        if (bytes < total) return fail(ASL_EINVAL, "dst too small: need %zu bytes", total);
        HIPCHK(hipMemcpy(dst, what == 0 ? d->qgray : d->dgray.p, total, hipMemcpyDeviceToHost));
        *n_items = total;
        return ASL_OK;
    }
    case 1: {
        if (bytes < total) return fail(ASL_EINVAL, "dst too small: need %zu bytes", total);
        if (int rc = expand_thresh(d, g, total)) return rc;
        HIPCHK(hipMemcpy(dst, d->dbg_thresh.p, total, hipMemcpyDeviceToHost));
        *n_items = total;
        return ASL_OK;
    }
    case 2: {  // labels live at run starts (run start -> tile-local root -> global root): resolve them per pixel for the caller
        if (bytes < total * 4) return fail(ASL_EINVAL, "dst too small: need %zu bytes", total * 4);
        if (d->dbg_labels.ensure(total)) return fail(ASL_ENOMEM, "debug buffer allocation failed");
        hipLaunchKernelGGL(k_seg_debug_labels, dim3((g.sw + 63) / 64, (g.sh + 3) / 4, (unsigned int)g.nframes), dim3(64, 4), 0, nullptr,
                           d->wmask.p, d->bmask.p, g, seg_nwx(g), d->parent.p, d->dbg_labels.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(dst, d->dbg_labels.p, total * 4, hipMemcpyDeviceToHost));
        *n_items = total;
        return ASL_OK;
    }
    case 3: {  // sizes are kept at the global roots; "no contrast" pixels are singletons whose size is implied
        if (bytes < total * 4) return fail(ASL_EINVAL, "dst too small: need %zu bytes", total * 4);
        if (int rc = expand_thresh(d, g, total)) return rc;
        std::vector<uint8_t> th(total);
        HIPCHK(hipMemcpy(th.data(), d->dbg_thresh.p, total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dst, d->sizes.p, total * 4, hipMemcpyDeviceToHost));
        unsigned int *o = (unsigned int *)dst;
        for (size_t i = 0; i < total; i++)
            if (th[i] == 127) o[i] = 1u;
        *n_items = total;
        return ASL_OK;
    }
    case 4: {  // the count is known once the records are on the host: checked there, before dst is written
        size_t ncl = (size_t)std::min<long long>(d->last_counters[CNT_NCLUSTERS], (long long)d->max_clusters);
        std::vector<QuadRec> q(ncl);
        if (ncl) HIPCHK(hipMemcpy(q.data(), d->quads.p, ncl * sizeof(QuadRec), hipMemcpyDeviceToHost));
        const size_t nvalid = (size_t)std::count_if(q.begin(), q.end(), [](const QuadRec &r) { return r.valid != 0; });
        if (bytes < nvalid * sizeof(asl_debug_quad))
            return fail(ASL_EINVAL, "dst too small: need %zu bytes for %zu quads", nvalid * sizeof(asl_debug_quad), nvalid);
        std::sort(q.begin(), q.end(), [](const QuadRec &a, const QuadRec &b) { return a.key < b.key; });
        asl_debug_quad *o = (asl_debug_quad *)dst;
        size_t k = 0;
        for (size_t i = 0; i < ncl; i++) {
            if (!q[i].valid) continue;
            for (int a = 0; a < 4; a++) { o[k].p[a][0] = q[i].p[a][0]; o[k].p[a][1] = q[i].p[a][1]; }
            unsigned long long key = q[i].key;
            o[k].frame = (int)(key >> 48);
            o[k].cluster = (((key >> 24) & 0xFFFFFFull) << 32) + (key & 0xFFFFFFull);
            o[k].reversed_border = q[i].reversed_border;
            k++;
        }
        *n_items = k;
        return ASL_OK;
    }
    case 5: {
        if (bytes < sizeof(long long) * 18) return fail(ASL_EINVAL, "dst too small: need %zu bytes", sizeof(long long) * 18);
        long long *o = (long long *)dst;
        o[0] = g.nframes; o[1] = g.sw; o[2] = g.sh;
        o[3] = d->last_counters[CNT_NCLUSTERS]; o[4] = d->last_counters[CNT_NPOINTS]; o[5] = d->last_counters[CNT_NQUADS];
        o[6] = d->last_counters[CNT_NDETS]; o[7] = d->nslots; o[8] = d->max_clusters; o[9] = d->max_points; o[10] = d->max_dets;
        o[11] = d->last_counters[CNT_OVERFLOW_HASH]; o[12] = d->last_counters[CNT_OVERFLOW_CLUSTERS];
        o[13] = d->last_counters[CNT_OVERFLOW_POINTS]; o[14] = d->last_counters[CNT_OVERFLOW_DETS]; o[15] = d->last_counters[CNT_CLASS0];
        o[16] = d->last_counters[CNT_DENSE_TILES]; o[17] = d->last_counters[CNT_DENSE_SEG];  // tiles that took the dense launches
        *n_items = 18;
        return ASL_OK;
    }
    case 6: {  // clusters as the quad fit receives them: (key, count, hash of the sorted point records), ordered by key
        size_t ncl = (size_t)std::min<long long>(d->last_counters[CNT_NCLUSTERS], (long long)d->max_clusters);
        size_t npts = (size_t)std::min<long long>(d->last_counters[CNT_NPOINTS], (long long)d->max_points);
        if (bytes < ncl * 24) return fail(ASL_EINVAL, "dst too small: need %zu bytes", ncl * 24);
        std::vector<ClusterRec> cl(ncl);
        std::vector<unsigned long long> pts(npts);
        if (ncl) HIPCHK(hipMemcpy(cl.data(), d->clusters.p, ncl * sizeof(ClusterRec), hipMemcpyDeviceToHost));
        if (npts) HIPCHK(hipMemcpy(pts.data(), d->points.p, npts * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::sort(cl.begin(), cl.end(), [](const ClusterRec &a, const ClusterRec &b) { return a.key < b.key; });
        unsigned long long *o = (unsigned long long *)dst;
        for (size_t i = 0; i < ncl; i++) {
            unsigned long long h = 0xcbf29ce484222325ull;
            if ((size_t)cl[i].offset + cl[i].count <= npts) {
                std::sort(pts.begin() + cl[i].offset, pts.begin() + cl[i].offset + cl[i].count);
                for (unsigned int k = 0; k < cl[i].count; k++) { h ^= pts[(size_t)cl[i].offset + k]; h *= 0x100000001b3ull; }
            }
            o[3 * i] = cl[i].key; o[3 * i + 1] = cl[i].count; o[3 * i + 2] = h;
        }
        *n_items = ncl;
        return ASL_OK;
    }
    default:
        return fail(ASL_EINVAL, "unknown debug item %d", what);
    }
}

// Run the quad fit of the last batch again, reps times, on the buffers it left behind; the fit is a pure function of the
// clusters, so any quad that comes out differently from the first repetition is a race.
extern "C" int asl_debug_refit(asl_detector *d, int reps, int64_t *out, size_t n_out)
{
    if (!d || !out) return fail(ASL_EINVAL, "NULL argument");
    if (reps < 1) return fail(ASL_EINVAL, "reps must be >= 1 (got %d)", reps);
    if (n_out < 2 + NCLASSES) return fail(ASL_EINVAL, "out too small: need %d values (got %zu)", 2 + NCLASSES, n_out);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    size_t ncl = (size_t)std::min<long long>(d->last_counters[CNT_NCLUSTERS], (long long)d->max_clusters);
    if (!ncl) return fail(ASL_EINVAL, "no clusters in the last batch");
    HIPCHK(hipSetDevice(d->device));
    const Geom &g = d->last;
    std::vector<QuadRec> ref(ncl), cur(ncl);
    std::vector<ClusterRec> cl(ncl);
    HIPCHK(hipMemcpy(cl.data(), d->clusters.p, ncl * sizeof(ClusterRec), hipMemcpyDeviceToHost));
    for (int k = 0; k < 2 + NCLASSES; k++) out[k] = 0;
    for (int r = 0; r < reps; r++) {
        // the all-LDS classes only: the global-slab class (more than 1024 points) sorts and de-duplicates inside its
        // clusters' point records, so a second run of it would not see the first one's input
        for (int cls = 0; cls < NCLASSES - 1; cls++) launch_fit_class(d, g, cls, (unsigned int)g.nframes, nullptr);
        launch_quad_finish(d, g, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy((r ? cur : ref).data(), d->quads.p, ncl * sizeof(QuadRec), hipMemcpyDeviceToHost));
        if (!r) continue;
        for (size_t i = 0; i < ncl; i++) {
            const bool same = cur[i].valid == ref[i].valid && (!ref[i].valid || memcmp(cur[i].p, ref[i].p, sizeof ref[i].p) == 0);
            if (same) continue;
            const unsigned int cnt = cl[i].count;
            if (cnt > CLASS3_CAP) continue;  // not re-run (above)
            out[1]++;
            out[2 + (cnt <= CLASS0_CAP ? 0 : (cnt <= CLASS1_CAP ? 1 : (cnt <= CLASS2_CAP ? 2 : (cnt <= CLASS3_CAP ? 3 : 4))))]++;
        }
    }
    out[0] = reps;
    return ASL_OK;
}

// S8 (k_dedup.inc) on the caller's records, through launch_dedup as a batch runs it, in device buffers of this call's own
// (freed on every path: DevBuf); the detector gives the device only.  One run, no growth: the counters say what a batch's
// host loop would have acted on.
extern "C" int asl_debug_dedup(asl_detector *d, const asl_detection *dets, const uint64_t *keys, int n, int n_frames, int cap_per_frame,
                               asl_detection *out, int max_out, int *n_per_frame, int64_t *counters, size_t n_counters)
{
    if (!d || !dets || !keys || !out || !n_per_frame || !counters) return fail(ASL_EINVAL, "NULL argument");
    if (n < 0) return fail(ASL_EINVAL, "n must be >= 0 (got %d)", n);
    if (n_frames < 1 || n_frames > 65535) return fail(ASL_EINVAL, "n_frames must be in [1, 65535] (got %d)", n_frames);
    if (cap_per_frame < 1) return fail(ASL_EINVAL, "cap_per_frame must be >= 1 (got %d)", cap_per_frame);
    if (max_out < n) return fail(ASL_EINVAL, "out too small: need %d records (got %d)", n, max_out);
    if (n_counters < 3) return fail(ASL_EINVAL, "counters too small: need 3 values (got %zu)", n_counters);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    for (int i = 0; i < n; i++)
        if (dets[i].frame < 0 || dets[i].frame >= n_frames)
            return fail(ASL_EINVAL, "record %d: frame %d is outside [0, %d)", i, dets[i].frame, n_frames);
    HIPCHK(hipSetDevice(d->device));
    const size_t B = (size_t)n_frames, nrec = (size_t)std::max(n, 1);
    std::vector<DetRec> h_recs(nrec);
    memset(h_recs.data(), 0, nrec * sizeof(DetRec));
    for (int i = 0; i < n; i++) {
        DetRec &r = h_recs[i];
        r.id = dets[i].id; r.hamming = dets[i].hamming; r.margin = dets[i].margin; r.frame = dets[i].frame;
        memcpy(r.center, dets[i].center, sizeof r.center);
        memcpy(r.corners, dets[i].corners, sizeof r.corners);
        r.key = ((uint64_t)dets[i].frame << 48) | (keys[i] & 0xFFFFFFFFFFFFull);  // a cluster key: the frame above 48 bits
    }
    DevBuf<DetRec> d_recs;
    DevBuf<long long> d_cnt;
    DevBuf<unsigned int> d_ndets, d_idx, d_nkeep, d_off;
    DevBuf<DetOut> d_out;
    if (d_recs.ensure(nrec) || d_cnt.ensure(CNT__N) || d_ndets.ensure(B) || d_idx.ensure(B * (size_t)cap_per_frame) || d_nkeep.ensure(B) ||
        d_off.ensure(B) || d_out.ensure(nrec))
        return fail(ASL_ENOMEM, "debug buffer allocation failed (%d records, %d frames of %d)", n, n_frames, cap_per_frame);
    std::vector<long long> h_cnt(CNT__N, 0);
    h_cnt[CNT_NDETS] = n;
    HIPCHK(hipMemcpy(d_recs.p, h_recs.data(), nrec * sizeof(DetRec), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cnt.p, h_cnt.data(), sizeof(long long) * CNT__N, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_ndets.p, 0, B * sizeof(unsigned int)));
    launch_dedup(S8Buffers{d_recs.p, d_cnt.p, (unsigned int)nrec, d_ndets.p, d_idx.p, (unsigned int)cap_per_frame, d_nkeep.p, d_off.p, d_out.p, nullptr},
                 (unsigned int)B, 0, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<unsigned int> h_nkeep(B);
    HIPCHK(hipMemcpy(h_cnt.data(), d_cnt.p, sizeof(long long) * CNT__N, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_nkeep.data(), d_nkeep.p, B * sizeof(unsigned int), hipMemcpyDeviceToHost));
    const long long nkeep = h_cnt[CNT_NKEEP];
    if (nkeep < 0 || nkeep > (long long)n) return fail(ASL_EDEVICE, "the de-duplication kept %lld of %d records", nkeep, n);
    static_assert(sizeof(DetOut) == sizeof(asl_detection), "device results are copied verbatim");
    if (nkeep) HIPCHK(hipMemcpy(out, d_out.p, (size_t)nkeep * sizeof(DetOut), hipMemcpyDeviceToHost));
    for (size_t f = 0; f < B; f++) n_per_frame[f] = (int)h_nkeep[f];
    counters[0] = nkeep; counters[1] = h_cnt[CNT_OVERFLOW_DETS]; counters[2] = h_cnt[CNT_DEDUP_LIMIT];
    return ASL_OK;
}

// The pose-graph back-end's dense linear algebra alone on the caller's matrix: gn_factor, the back substitution and k_map_std
// as asl_gn_solve and the map solver enqueue them (gn_host.inc, launch_map), in device buffers of this call's own.
extern "C" int asl_debug_gn_cholesky(asl_detector *d, const double *A, const double *b, int n, double *L, size_t n_L, double *y, double *x,
                                     double *var, size_t n_vec, double *Linv, size_t n_Linv, int32_t *fail_flag)
{
    if (!d || !A || !b || !L || !y || !x || !var || !Linv || !fail_flag) return fail(ASL_EINVAL, "NULL argument");
    if (n < 6 || n > 6000 || n % 6) return fail(ASL_EINVAL, "n must be 6 times a tag count in [1, 1000] (got %d)", n);
    const size_t N = (size_t)n, nblk = (N + GN_NB - 1) / GN_NB, nli = nblk * GN_NB * GN_NB;
    if (n_L < N * N) return fail(ASL_EINVAL, "L too small: need %zu values (got %zu)", N * N, n_L);
    if (n_vec < N) return fail(ASL_EINVAL, "y, x and var too small: need %zu values each (got %zu)", N, n_vec);
    if (n_Linv < nli) return fail(ASL_EINVAL, "Linv too small: need %zu values (got %zu)", nli, n_Linv);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    HIPCHK(hipSetDevice(d->device));
    DevBuf<double> d_S, d_x, d_Linv, d_var;
    DevBuf<int> d_flag;
    if (d_S.ensure((N + 1) * N) || d_x.ensure(N) || d_Linv.ensure(nli) || d_var.ensure(N) || d_flag.ensure(1))
        return fail(ASL_ENOMEM, "debug buffer allocation failed (n = %d)", n);
    HIPCHK(hipMemcpy(d_S.p, A, N * N * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_S.p + N * N, b, N * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_flag.p, 0, sizeof(int)));
    gn_factor(d_S.p, d_Linv.p, n, d_flag.p, nullptr);
    gn_trisolve(d_S.p, d_Linv.p, d_x.p, n, nullptr);
    hipLaunchKernelGGL(k_map_std, dim3(n), dim3(256), N * sizeof(double), nullptr, d_S.p, d_Linv.p, n, d_var.p);
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpy(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(L, d_S.p, N * N * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < N; r++)
        for (size_t c = r + 1; c < N; c++) L[r * N + c] = 0.0;  // the factorisation leaves A's upper triangle there
    HIPCHK(hipMemcpy(y, d_S.p + N * N, N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(x, d_x.p, N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(var, d_var.p, N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(Linv, d_Linv.p, nli * sizeof(double), hipMemcpyDeviceToHost));
    *fail_flag = flag;
    return ASL_OK;
}

// One damped step of asl_gn_solve's problem, stage by stage: the linearisation and its cost, gn_eliminate, gn_factor and
// gn_step as gn_factor_step runs them, S and rhs read back between the first two.  A workspace of this call's own.
extern "C" int asl_debug_gn_step(asl_detector *d, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam, const int32_t *obs_tag,
                                 const double *obs_corners, const double *K, double tag_size, int fixed_tag, const double *cam_T,
                                 const double *tag_T, double lambda, const asl_debug_span *out, int n_out, int32_t *fail_flag)
{
    GnHostProblem h;
    if (int rc = gn_host_problem(d, n_cams, n_tags, n_obs, obs_cam, obs_tag, obs_corners, K, fixed_tag, cam_T, tag_T, h)) return rc;
    if (!out) return fail(ASL_EINVAL, "NULL argument");
    if (!(lambda >= 0) || !std::isfinite(lambda)) return fail(ASL_EINVAL, "lambda must be >= 0 and finite (got %g)", lambda);
    if (n_out != ASL_GN_STEP__N) return fail(ASL_EINVAL, "out must have %d entries (got %d)", ASL_GN_STEP__N, n_out);
    const size_t nc = (size_t)n_cams, nt = (size_t)n_tags, nm = (size_t)n_obs, n = 6 * nt;
    const size_t need[ASL_GN_STEP__N] = {GN_DSTRIDE * nm, nm, 1, 36 * nc, 6 * nc, 36 * nm, n * n, n, n, 12 * nc, 12 * nt};
    for (int i = 0; i < ASL_GN_STEP__N; i++)
        if (out[i].p && out[i].n < need[i]) return fail(ASL_EINVAL, "out[%d] too small: need %zu values (got %zu)", i, need[i], out[i].n);
    if (d->pending) return fail(ASL_EINVAL, "a batch is in flight on this detector");
    HIPCHK(hipSetDevice(d->device));
    DevBuf<uint8_t> ws;
    GnDevProblem p;
    if (int rc = gn_stage_problem(ws, h, n_cams, n_tags, n_obs, obs_cam, obs_tag, obs_corners, fixed_tag, nullptr, p)) return rc;
    const GnSystem &sys = p.sys;
    double lm_init[GN_LM__N] = {0, 0, lambda, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpy(p.b.lm, lm_init, sizeof lm_init, hipMemcpyHostToDevice));
    const CamDev cam = make_cam(d, K, nullptr, 0, tag_size);
    gn_launch_linearize(p, cam, n_obs, p.Wc, p.Gc, sys.D, nullptr);
    hipLaunchKernelGGL(k_gn_cost, dim3(1), dim3(256), 0, nullptr, p.b.cost_obs, n_obs, p.b.lm + GN_LM_COST);
    if (int rc = gn_eliminate(sys, p.b.lm, nullptr)) return rc;
    HIPCHK(hipGetLastError());
    auto fetch = [&](int item, const double *src) {
        return out[item].p ? hipMemcpy(out[item].p, src, need[item] * sizeof(double), hipMemcpyDeviceToHost) : hipSuccess;
    };
    HIPCHK(fetch(ASL_GN_STEP_S, sys.S));
    HIPCHK(fetch(ASL_GN_STEP_RHS, sys.rhs));
    gn_factor(sys.S, sys.Linv, (int)n, p.b.flag, nullptr);
    gn_step(sys, nullptr, p.Wc, p.Gc, p.b.Wn, p.b.Gn);
    HIPCHK(hipGetLastError());
    HIPCHK(fetch(ASL_GN_STEP_D, sys.D));
    HIPCHK(fetch(ASL_GN_STEP_COST_OBS, p.b.cost_obs));
    HIPCHK(fetch(ASL_GN_STEP_COST, p.b.lm + GN_LM_COST));
    HIPCHK(fetch(ASL_GN_STEP_HINV, sys.Hinv));
    HIPCHK(fetch(ASL_GN_STEP_GC, sys.gc));
    HIPCHK(fetch(ASL_GN_STEP_TFJ, sys.Tfj));
    HIPCHK(fetch(ASL_GN_STEP_DG, sys.rhs));
    HIPCHK(fetch(ASL_GN_STEP_WN, p.b.Wn));
    HIPCHK(fetch(ASL_GN_STEP_GN, p.b.Gn));
    if (fail_flag) {
        int flag = 0;
        HIPCHK(hipMemcpy(&flag, p.b.flag, sizeof(int), hipMemcpyDeviceToHost));
        *fail_flag = flag;
    }
    return ASL_OK;
}

extern "C" int asl_debug_division_check(asl_detector *d, int exponent_limit, int64_t *out, size_t n_out)
{
    if (!d || !out) return fail(ASL_EINVAL, "NULL argument");
    if (exponent_limit < 1 || exponent_limit > 900) return fail(ASL_EINVAL, "exponent_limit must be in [1, 900] (got %d)", exponent_limit);
    if (n_out < 2) return fail(ASL_EINVAL, "out too small: need 2 values (got %zu)", n_out);
    HIPCHK(hipSetDevice(d->device));
    const int blocks = 2048, per = 1024;
    DevBuf<unsigned long long> d_bad;  // freed on every path
    if (d_bad.ensure(1)) return fail(ASL_ENOMEM, "debug buffer allocation failed");
    HIPCHK(hipMemset(d_bad.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(k_div_check, dim3(blocks), dim3(256), 0, nullptr, 20260301ull, per, exponent_limit, d_bad.p);
    HIPCHK(hipGetLastError());
    unsigned long long h_bad = 0;
    HIPCHK(hipMemcpy(&h_bad, d_bad.p, sizeof h_bad, hipMemcpyDeviceToHost));
    out[0] = (int64_t)blocks * 256 * per;
    out[1] = (int64_t)h_bad;
    return ASL_OK;
}

extern "C" int asl_debug_phase_cycles(asl_detector *d, unsigned long long *out, size_t n_out, int reset)
{
    if (!d || !out) return fail(ASL_EINVAL, "NULL argument");
    if (n_out < 64) return fail(ASL_EINVAL, "out too small: need 64 values (got %zu)", n_out);
    HIPCHK(hipSetDevice(d->device));
    std::vector<unsigned long long> all((size_t)64 * PHASE_SPREAD);
    HIPCHK(hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(g_phase_cycles), sizeof(unsigned long long) * all.size()));
    for (int i = 0; i < 64; i++) {
        out[i] = 0;
        for (int k = 0; k < PHASE_SPREAD; k++) out[i] += all[(size_t)i * PHASE_SPREAD + k];
    }
    if (reset) {
        std::fill(all.begin(), all.end(), 0ull);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), all.data(), sizeof(unsigned long long) * all.size()));
    }
    return ASL_OK;
}
