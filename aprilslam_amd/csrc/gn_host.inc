// Host side of the pose-graph Levenberg-Marquardt back-end (kernels: k_gn.inc): the LM's buffers, the reduced-system
// sequence and the trial loop that asl_gn_solve and the map solver (k_map.inc, launch_map) share, and asl_gn_solve itself.

// One problem's reduced system on the device: observation blocks D, the active lists and (camera, tag) table, scratch
struct GnSystem {
    double *D;
    int *cam_ptr, *cam_obs, *tag_ptr, *tag_obs, *obs_cam, *obs_tag, *obs_of;
    int n_cams, n_tags, fixed_tag;
    double *Hinv, *gc, *Tfj, *S, *rhs, *Linv;
};

// The three pieces of one damped step, each enqueued on st; gn_factor_step calls them in order, and a diagnostic
// (debug_host.inc) may read S between the first two or hand gn_factor a matrix of its own.
// Eliminate: the cameras reduced out (damping: lm[GN_LM_LAMBDA]), the Schur complement S over the tags and its right-hand
// side, which is copied into row n of S
static int gn_eliminate(const GnSystem &g, const double *lm, hipStream_t st)
{
    const int n = 6 * g.n_tags;
    hipLaunchKernelGGL(k_gn_reduce_cam, dim3(g.n_cams), dim3(64), 0, st, g.D, g.cam_ptr, g.cam_obs, g.n_cams, lm, g.Hinv, g.gc, g.Tfj);
    hipLaunchKernelGGL(k_gn_schur, dim3(g.n_tags, g.n_tags), dim3(64), 0, st, g.D, g.Tfj, g.Hinv, g.gc, g.tag_ptr, g.tag_obs, g.obs_cam,
                       g.obs_of, g.n_cams, g.n_tags, g.fixed_tag, lm, g.S, g.rhs);
    HIPCHK(hipMemcpyAsync(g.S + (size_t)n * n, g.rhs, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    return ASL_OK;
}

// Factor: the blocked Cholesky of S ((n + 1) x n, row n the right-hand side, which leaves as L^-1 b) in place, the inverses
// of the diagonal blocks into Linv; fail_flag set if S is not positive definite
static void gn_factor(double *S, double *Linv, int n, int *fail_flag, hipStream_t st)
{
    for (int k0 = 0; k0 < n; k0 += GN_NB) {
        const int nb = std::min(GN_NB, n - k0), rem = n + 1 - k0 - nb;  // rows below the block, including row n
        hipLaunchKernelGGL(k_gn_chol_diag, dim3(1), dim3(64), 0, st, S, n, k0, nb, fail_flag, Linv);
        hipLaunchKernelGGL(k_gn_chol_panel, dim3((rem + 15) / 16), dim3(256), 0, st, S, n, n + 1, k0, nb);
        if (rem > 1) {
            const unsigned int tiles = (unsigned int)((rem + GN_NB - 1) / GN_NB);
            hipLaunchKernelGGL(k_gn_chol_update, dim3(tiles, tiles), dim3(256), 0, st, S, n, n + 1, k0, nb);
        }
    }
}

// the back substitution L^T x = (row n of S) into x (n doubles)
static void gn_trisolve(const double *S, const double *Linv, double *x, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_gn_trisolve, dim3(1), dim3(GN_TRI_THREADS), (size_t)n * sizeof(double), st, S, Linv, x, n);
}

// Step: the back substitution (the tag steps, into g.rhs), the camera steps and the trial poses (Wn, Gn) from (W, G)
static void gn_step(const GnSystem &g, hipStream_t st, const double *W, const double *G, double *Wn, double *Gn)
{
    gn_trisolve(g.S, g.Linv, g.rhs, 6 * g.n_tags, st);
    hipLaunchKernelGGL(k_gn_update, dim3((g.n_cams + g.n_tags + 63) / 64), dim3(64), 0, st, g.D, g.Hinv, g.gc, g.cam_ptr, g.cam_obs,
                       g.obs_tag, g.rhs, g.n_cams, g.n_tags, W, G, Wn, Gn);
}

// Enqueued on st: eliminate and factor (fail set if the reduced system is not positive definite); with Wn, also the step
static int gn_factor_step(const GnSystem &g, const double *lm, int *fail_flag, hipStream_t st, const double *W = nullptr,
                          const double *G = nullptr, double *Wn = nullptr, double *Gn = nullptr)
{
    if (int rc = gn_eliminate(g, lm, st)) return rc;
    gn_factor(g.S, g.Linv, 6 * g.n_tags, fail_flag, st);
    if (Wn) gn_step(g, st, W, G, Wn, Gn);
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

// A pose-graph problem as the ABI states it, checked and put into the kernels' form on the host: the CSR lists by camera
// and by tag (observation order kept), the (camera, tag) -> observation table, the poses packed (W camera<-world, G)
struct GnHostProblem {
    std::vector<int> cam_ptr, tag_ptr, cam_obs, tag_obs, obs_of;
    std::vector<double> W, G;
};

static int gn_host_problem(const asl_detector *d, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam, const int32_t *obs_tag,
                           const double *obs_corners, const double *K, int fixed_tag, const double *cam_T, const double *tag_T,
                           GnHostProblem &h)
{
    if (!d || !obs_cam || !obs_tag || !obs_corners || !K || !cam_T || !tag_T) return fail(ASL_EINVAL, "NULL argument");
    if (n_cams <= 0 || n_tags <= 0 || n_obs <= 0) return fail(ASL_EINVAL, "empty problem");
    if (fixed_tag < 0 || fixed_tag >= n_tags) return fail(ASL_EINVAL, "fixed_tag out of range");
    if ((long long)n_tags * 6 > 6000) return fail(ASL_EINVAL, "more than 1000 tags: the dense reduced system is not meant for that");
    h.cam_ptr.assign(n_cams + 1, 0); h.tag_ptr.assign(n_tags + 1, 0); h.cam_obs.resize(n_obs); h.tag_obs.resize(n_obs);
    h.obs_of.assign((size_t)n_cams * n_tags, -1);
    for (int m = 0; m < n_obs; m++) {
        int f = obs_cam[m], j = obs_tag[m];
        if (f < 0 || f >= n_cams || j < 0 || j >= n_tags) return fail(ASL_EINVAL, "observation %d references camera %d / tag %d", m, f, j);
        if (h.obs_of[(size_t)f * n_tags + j] >= 0) return fail(ASL_EINVAL, "camera %d observes tag %d twice", f, j);
        h.obs_of[(size_t)f * n_tags + j] = m;
        h.cam_ptr[f + 1]++; h.tag_ptr[j + 1]++;
    }
    for (int f = 0; f < n_cams; f++) h.cam_ptr[f + 1] += h.cam_ptr[f];
    for (int j = 0; j < n_tags; j++) h.tag_ptr[j + 1] += h.tag_ptr[j];
    {
        std::vector<int> cf(h.cam_ptr.begin(), h.cam_ptr.end() - 1), tf(h.tag_ptr.begin(), h.tag_ptr.end() - 1);
        for (int m = 0; m < n_obs; m++) { h.cam_obs[cf[obs_cam[m]]++] = m; h.tag_obs[tf[obs_tag[m]]++] = m; }
    }
    h.W.resize((size_t)12 * n_cams); h.G.resize((size_t)12 * n_tags);
    for (int f = 0; f < n_cams; f++) gn_rigid_inverse(cam_T + 16 * (size_t)f, &h.W[12 * (size_t)f]);
    for (int j = 0; j < n_tags; j++) gn_pack(tag_T + 16 * (size_t)j, &h.G[12 * (size_t)j]);
    return ASL_OK;
}

// The problem on the device, in one workspace: the inputs (poses, corners, observation lists and their CSR) and the LM's
// buffers; the uploads are enqueued on st and the LM's failure flag cleared
struct GnDevProblem {
    GnSystem sys{};
    double *Wc, *Gc, *corners;
    GnLmBufs b;
};

static int gn_stage_problem(DevBuf<uint8_t> &ws, const GnHostProblem &h, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam,
                            const int32_t *obs_tag, const double *obs_corners, int fixed_tag, hipStream_t st, GnDevProblem &p)
{
    GnSystem &sys = p.sys;
    sys.n_cams = n_cams; sys.n_tags = n_tags; sys.fixed_tag = fixed_tag;
    if (carve_ws(ws, [&](WsCarve &c) {
            p.Wc = c.take<double>(h.W.size()); p.Gc = c.take<double>(h.G.size()); p.corners = c.take<double>((size_t)8 * n_obs);
            sys.obs_cam = c.take<int>(n_obs); sys.obs_tag = c.take<int>(n_obs); sys.cam_ptr = c.take<int>(h.cam_ptr.size());
            sys.cam_obs = c.take<int>(n_obs); sys.tag_ptr = c.take<int>(h.tag_ptr.size()); sys.tag_obs = c.take<int>(n_obs);
            p.b = gn_lm_carve(c, sys, n_obs, GN_LM__N);
        }))
        return fail(ASL_ENOMEM, "Gauss-Newton workspace allocation failed");
    HIPCHK(hipMemcpyAsync(p.Wc, h.W.data(), h.W.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p.Gc, h.G.data(), h.G.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(p.corners, obs_corners, (size_t)8 * n_obs * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_cam, obs_cam, (size_t)n_obs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_tag, obs_tag, (size_t)n_obs * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.cam_ptr, h.cam_ptr.data(), h.cam_ptr.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.cam_obs, h.cam_obs.data(), h.cam_obs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.tag_ptr, h.tag_ptr.data(), h.tag_ptr.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.tag_obs, h.tag_obs.data(), h.tag_obs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.obs_of, h.obs_of.data(), h.obs_of.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(p.b.flag, 0, 4, st));
    return ASL_OK;
}

static void gn_launch_linearize(const GnDevProblem &p, const CamDev &cam, int n_obs, const double *Wp, const double *Gp, double *Dp,
                                hipStream_t st)
{
    hipLaunchKernelGGL(k_gn_linearize, dim3((n_obs + 3) / 4), dim3(256), 0, st, Wp, Gp, p.sys.obs_cam, p.sys.obs_tag, p.corners, n_obs, cam, Dp,
                       p.b.cost_obs);
}

extern "C" int asl_gn_solve(asl_detector *d, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam, const int32_t *obs_tag,
                            const double *obs_corners, const double *K, double tag_size, int fixed_tag, double *cam_T,
                            double *tag_T, int iters, double *stats)
{
    GnHostProblem h;
    if (int rc = gn_host_problem(d, n_cams, n_tags, n_obs, obs_cam, obs_tag, obs_corners, K, fixed_tag, cam_T, tag_T, h)) return rc;
    if (iters < 0) return fail(ASL_EINVAL, "iters must be >= 0 (got %d)", iters);
    HIPCHK(hipSetDevice(d->device));
    // a stream of its own, at the highest priority: the solve is a chain of small launches and read-backs, and behind a
    // detector batch on a shared queue every one of them would wait for the whole batch
    if (!d->aux_stream) {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&d->aux_stream, hipStreamNonBlocking, hi));
    }
    hipStream_t st = d->aux_stream;
    GnDevProblem p;
    if (int rc = gn_stage_problem(d->gn_ws, h, n_cams, n_tags, n_obs, obs_cam, obs_tag, obs_corners, fixed_tag, st, p)) return rc;
    const GnSystem &sys = p.sys;
    const GnLmBufs &b = p.b;
    double *Wc = p.Wc, *Gc = p.Gc;
    std::vector<double> &W = h.W, &G = h.G;

    const CamDev cam = make_cam(d, K, nullptr, 0, tag_size);
    auto lin = [&](const double *Wp, const double *Gp, double *Dp, int) { gn_launch_linearize(p, cam, n_obs, Wp, Gp, Dp, st); };
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
