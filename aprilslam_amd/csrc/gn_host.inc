// Host side of the pose-graph Levenberg-Marquardt back-end (kernels: k_gn.inc): the LM's buffers, the reduced-system
// sequence and the trial loop that asl_gn_solve and the map solver (k_map.inc, launch_map) share, and asl_gn_solve itself.

// One problem's reduced system on the device: observation blocks D, the active lists and (camera, tag) table, scratch
struct GnSystem {
    double *D;
    int *cam_ptr, *cam_obs, *tag_ptr, *tag_obs, *obs_cam, *obs_tag, *obs_of;
    int n_cams, n_tags, fixed_tag;
    double *Hinv, *gc, *Tfj, *S, *rhs, *Linv;
};

// Enqueued on st: the cameras eliminated and the Schur complement over the tags (damping: lm[GN_LM_LAMBDA]), its blocked
// Cholesky with the right-hand side carried as row n (fail set if it is not positive definite); with Wn, also the step:
// the triangular solves and the trial poses (Wn, Gn) from (W, G)
static int gn_factor_step(const GnSystem &g, const double *lm, int *fail_flag, hipStream_t st, const double *W = nullptr,
                          const double *G = nullptr, double *Wn = nullptr, double *Gn = nullptr)
{
    const int n = 6 * g.n_tags;
    hipLaunchKernelGGL(k_gn_reduce_cam, dim3(g.n_cams), dim3(64), 0, st, g.D, g.cam_ptr, g.cam_obs, g.n_cams, lm, g.Hinv, g.gc, g.Tfj);
    hipLaunchKernelGGL(k_gn_schur, dim3(g.n_tags, g.n_tags), dim3(64), 0, st, g.D, g.Tfj, g.Hinv, g.gc, g.tag_ptr, g.tag_obs, g.obs_cam,
                       g.obs_of, g.n_cams, g.n_tags, g.fixed_tag, lm, g.S, g.rhs);
    HIPCHK(hipMemcpyAsync(g.S + (size_t)n * n, g.rhs, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    for (int k0 = 0; k0 < n; k0 += GN_NB) {
        const int nb = std::min(GN_NB, n - k0), rem = n + 1 - k0 - nb;  // rows below the block, including row n
        hipLaunchKernelGGL(k_gn_chol_diag, dim3(1), dim3(64), 0, st, g.S, n, k0, nb, fail_flag, g.Linv);
        hipLaunchKernelGGL(k_gn_chol_panel, dim3((rem + 15) / 16), dim3(256), 0, st, g.S, n, n + 1, k0, nb);
        if (rem > 1) {
            const unsigned int tiles = (unsigned int)((rem + GN_NB - 1) / GN_NB);
            hipLaunchKernelGGL(k_gn_chol_update, dim3(tiles, tiles), dim3(256), 0, st, g.S, n, n + 1, k0, nb);
        }
    }
    if (!Wn) return ASL_OK;
    hipLaunchKernelGGL(k_gn_trisolve, dim3(1), dim3(GN_TRI_THREADS), (size_t)n * sizeof(double), st, g.S, g.Linv, g.rhs, n);
    hipLaunchKernelGGL(k_gn_update, dim3((g.n_cams + g.n_tags + 63) / 64), dim3(64), 0, st, g.D, g.Hinv, g.gc, g.cam_ptr, g.cam_obs,
                       g.obs_tag, g.rhs, g.n_cams, g.n_tags, W, G, Wn, Gn);
    return ASL_OK;
}

// The LM's buffers beside the reduced system: two failure flags (the LM's factorisation, and one for the caller), the LM
// state (n_lm doubles), trial poses and blocks, per-observation costs.  gn_lm_carve carves them and the reduced system's
// problem-sized ones (blocks D, (camera, tag) table, scratch) for sys.n_cams cameras and sys.n_tags tags.
struct GnLmBufs {
    int *flag;
    double *lm, *Wn, *Gn, *Dn, *cost_obs;
};

static GnLmBufs gn_lm_carve(WsCarve &c, GnSystem &sys, int n_obs, int n_lm)
{
    const size_t nc = (size_t)sys.n_cams, nt = (size_t)sys.n_tags, nm = (size_t)n_obs, n = 6 * nt;
    GnLmBufs b;
    sys.obs_of = c.take<int>(nc * nt); b.flag = c.take<int>(2); b.lm = c.take<double>((size_t)n_lm);
    b.Wn = c.take<double>(12 * nc); b.Gn = c.take<double>(12 * nt);
    sys.D = c.take<double>(GN_DSTRIDE * nm); b.Dn = c.take<double>(GN_DSTRIDE * nm); b.cost_obs = c.take<double>(nm);
    sys.Hinv = c.take<double>(36 * nc); sys.gc = c.take<double>(6 * nc); sys.Tfj = c.take<double>(36 * nm);
    sys.S = c.take<double>((n + 1) * n);  // row n carries the right-hand side through the factorisation
    sys.rhs = c.take<double>(n); sys.Linv = c.take<double>((n + GN_NB - 1) / GN_NB * GN_NB * GN_NB);
    return b;
}

// The LM, all enqueued on st: the current state (W, G, sys.D) linearised and costed (lm[GN_LM_COST], and COST0; its
// per-observation costs also to seed_obs, if given), then iters trials: the damped step into (b.Wn, b.Gn), linearised into
// b.Dn, costed (lm[GN_LM_TRIAL]), decided and committed.  lin(W, G, D, force) enqueues a linearisation into D and
// b.cost_obs, decide() the accept rule, tail() whatever follows a trial.
template <class Lin, class Decide, class Tail>
static int gn_lm_run(const GnSystem &sys, const GnLmBufs &b, double *W, double *G, int n_obs, int iters, double *seed_obs, Lin lin,
                     Decide decide, Tail tail, hipStream_t st)
{
    lin(W, G, sys.D, 1);
    hipLaunchKernelGGL(k_gn_cost, dim3(1), dim3(256), 0, st, b.cost_obs, n_obs, b.lm + GN_LM_COST);
    HIPCHK(hipMemcpyAsync(b.lm + GN_LM_COST0, b.lm + GN_LM_COST, 8, hipMemcpyDeviceToDevice, st));
    if (seed_obs) HIPCHK(hipMemcpyAsync(seed_obs, b.cost_obs, 8 * (size_t)n_obs, hipMemcpyDeviceToDevice, st));
    const size_t nw = (size_t)12 * sys.n_cams, ng = (size_t)12 * sys.n_tags, nd = (size_t)GN_DSTRIDE * n_obs;
    const unsigned int commit_blocks = (unsigned int)std::min<size_t>((nw + ng + nd + 255) / 256, 1024);
    for (int it = 0; it < iters; it++) {
        int rc = gn_factor_step(sys, b.lm, b.flag, st, W, G, b.Wn, b.Gn);
        if (rc) return rc;
        lin(b.Wn, b.Gn, b.Dn, 0);
        hipLaunchKernelGGL(k_gn_cost, dim3(1), dim3(256), 0, st, b.cost_obs, n_obs, b.lm + GN_LM_TRIAL);
        decide();
        hipLaunchKernelGGL(k_gn_commit, dim3(commit_blocks), dim3(256), 0, st, b.lm, b.Wn, b.Gn, b.Dn, W, G, sys.D, nw, ng, nd);
        tail();
    }
    return ASL_OK;
}

static void gn_rigid_inverse(const double *T, double *W12)
{
    // T = [R t; 0 1] row-major 4x4  ->  W = [R^T, -R^T t] packed as R(9) t(3)
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) W12[3 * r + c] = T[4 * c + r];
    for (int r = 0; r < 3; r++) W12[9 + r] = -(W12[3 * r] * T[3] + W12[3 * r + 1] * T[7] + W12[3 * r + 2] * T[11]);
}

static void gn_pack(const double *T, double *P12)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) P12[3 * r + c] = T[4 * r + c];
        P12[9 + r] = T[4 * r + 3];
    }
}

static void gn_unpack(const double *P12, double *T)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = P12[3 * r + c];
        T[4 * r + 3] = P12[9 + r];
    }
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

extern "C" int asl_gn_solve(asl_detector *d, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam, const int32_t *obs_tag,
                            const double *obs_corners, const double *K, double tag_size, int fixed_tag, double *cam_T,
                            double *tag_T, int iters, double *stats)
{
    if (!d || !obs_cam || !obs_tag || !obs_corners || !K || !cam_T || !tag_T) return fail(ASL_EINVAL, "NULL argument");
    if (n_cams <= 0 || n_tags <= 0 || n_obs <= 0 || iters < 0) return fail(ASL_EINVAL, "empty problem");
    if (fixed_tag < 0 || fixed_tag >= n_tags) return fail(ASL_EINVAL, "fixed_tag out of range");
    if ((long long)n_tags * 6 > 6000) return fail(ASL_EINVAL, "more than 1000 tags: the dense reduced system is not meant for that");
    HIPCHK(hipSetDevice(d->device));

    // CSR lists by camera and by tag (observation order kept), and the (camera, tag) -> observation table
    std::vector<int> cam_ptr(n_cams + 1, 0), tag_ptr(n_tags + 1, 0), cam_obs(n_obs), tag_obs(n_obs), obs_of((size_t)n_cams * n_tags, -1);
    for (int m = 0; m < n_obs; m++) {
        int f = obs_cam[m], j = obs_tag[m];
        if (f < 0 || f >= n_cams || j < 0 || j >= n_tags) return fail(ASL_EINVAL, "observation %d references camera %d / tag %d", m, f, j);
        if (obs_of[(size_t)f * n_tags + j] >= 0) return fail(ASL_EINVAL, "camera %d observes tag %d twice", f, j);
        obs_of[(size_t)f * n_tags + j] = m;
        cam_ptr[f + 1]++; tag_ptr[j + 1]++;
    }
    for (int f = 0; f < n_cams; f++) cam_ptr[f + 1] += cam_ptr[f];
    for (int j = 0; j < n_tags; j++) tag_ptr[j + 1] += tag_ptr[j];
    {
        std::vector<int> cf(cam_ptr.begin(), cam_ptr.end() - 1), tf(tag_ptr.begin(), tag_ptr.end() - 1);
        for (int m = 0; m < n_obs; m++) { cam_obs[cf[obs_cam[m]]++] = m; tag_obs[tf[obs_tag[m]]++] = m; }
    }
    std::vector<double> W((size_t)12 * n_cams), G((size_t)12 * n_tags);
    for (int f = 0; f < n_cams; f++) gn_rigid_inverse(cam_T + 16 * (size_t)f, &W[12 * (size_t)f]);
    for (int j = 0; j < n_tags; j++) gn_pack(tag_T + 16 * (size_t)j, &G[12 * (size_t)j]);

    // one workspace: the inputs (poses, corners, observation lists and their CSR) and the LM's buffers
    GnSystem sys{};
    sys.n_cams = n_cams; sys.n_tags = n_tags; sys.fixed_tag = fixed_tag;
    double *Wc, *Gc, *corners;
    GnLmBufs b;
    if (carve_ws(d->gn_ws, [&](WsCarve &c) {
            Wc = c.take<double>(W.size()); Gc = c.take<double>(G.size()); corners = c.take<double>((size_t)8 * n_obs);
            sys.obs_cam = c.take<int>(n_obs); sys.obs_tag = c.take<int>(n_obs); sys.cam_ptr = c.take<int>(cam_ptr.size());
            sys.cam_obs = c.take<int>(n_obs); sys.tag_ptr = c.take<int>(tag_ptr.size()); sys.tag_obs = c.take<int>(n_obs);
            b = gn_lm_carve(c, sys, n_obs, GN_LM__N);
        }))
        return fail(ASL_ENOMEM, "Gauss-Newton workspace allocation failed");
    // a stream of its own, at the highest priority: the solve is a chain of small launches and read-backs, and behind a
    // detector batch on a shared queue every one of them would wait for the whole batch
    if (!d->aux_stream) {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&d->aux_stream, hipStreamNonBlocking, hi));
    }
    hipStream_t st = d->aux_stream;
    HIPCHK(hipMemcpyAsync(Wc, W.data(), W.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(Gc, G.data(), G.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(corners, obs_corners, (size_t)8 * n_obs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_cam, obs_cam, (size_t)n_obs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_tag, obs_tag, (size_t)n_obs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.cam_ptr, cam_ptr.data(), cam_ptr.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.cam_obs, cam_obs.data(), cam_obs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.tag_ptr, tag_ptr.data(), tag_ptr.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.tag_obs, tag_obs.data(), tag_obs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_of, obs_of.data(), obs_of.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b.flag, 0, 4, st));

    const CamDev cam = make_cam(d, K, nullptr, 0, tag_size);
    auto lin = [&](const double *Wp, const double *Gp, double *Dp, int) {
        hipLaunchKernelGGL(k_gn_linearize, dim3((n_obs + 3) / 4), dim3(256), 0, st, Wp, Gp, sys.obs_cam, sys.obs_tag, corners, n_obs, cam, Dp, b.cost_obs);
    };
    auto decide = [&]() { hipLaunchKernelGGL(k_gn_decide, dim3(1), dim3(1), 0, st, b.lm); };
    // The whole solve is enqueued at once: cost, lambda and the accept / reject decision live in device memory (b.lm), an
    // accepted trial is copied over the current state, and the host waits exactly once, at the end.
    range_push("G pose-graph LM");
    double lm_init[GN_LM__N] = {0, 0, 1e-3, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(b.lm, lm_init, sizeof lm_init, hipMemcpyHostToDevice, st));
    int rc = gn_lm_run(sys, b, Wc, Gc, n_obs, iters, nullptr, lin, decide, [] {}, st);
    if (rc) return rc;
    double lm[GN_LM__N];
    HIPCHK(hipMemcpyAsync(lm, b.lm, sizeof lm, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, b.flag, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(W.data(), Wc, W.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(G.data(), Gc, G.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    range_pop();
    for (int f = 0; f < n_cams; f++) {
        double T[16], Wi[12];
        gn_unpack(&W[12 * (size_t)f], T);
        gn_rigid_inverse(T, Wi);
        gn_unpack(Wi, cam_T + 16 * (size_t)f);
    }
    for (int j = 0; j < n_tags; j++) gn_unpack(&G[12 * (size_t)j], tag_T + 16 * (size_t)j);
    if (stats) { stats[0] = lm[GN_LM_COST0]; stats[1] = lm[GN_LM_COST]; stats[2] = lm[GN_LM_ACCEPTED]; }
    if (flag) return fail(ASL_EINVAL, "reduced system not positive definite (under-constrained problem?)");
    return ASL_OK;
}
