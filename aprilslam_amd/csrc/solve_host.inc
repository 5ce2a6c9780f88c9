// Host side of the device solvers on asl_obs blocks: localisation and rig localisation (kernels: k_localize.inc, k_rig.inc),
// per-tag pose covariance (k_posecov.inc), calibration (k_calib.inc), rig mounting calibration (k_rigcal.inc), mapping (k_map.inc), sequence smoothing
// (k_smooth.inc) and tag location (k_locate.inc).  Every solver has one call record, filled by its extern "C" entry points in their argument order, one
// check_*_call with every refusal, one launch_* on device pointers, one device form and one host form.  The host forms
// share stage_host_call (the block and the map in, the results carved from d->solve_out) and fetch_out (the results back).

static_assert(sizeof(MapTagRec) == sizeof(asl_map_tag) && sizeof(asl_map_tag) == 104, "asl_map_tag layout");
static_assert(sizeof(CamPoseRec) == sizeof(asl_cam_pose) && sizeof(asl_cam_pose) == 160, "asl_cam_pose layout");
static_assert(sizeof(PoseCovRec) == sizeof(asl_pose_cov) && sizeof(asl_pose_cov) == 304, "asl_pose_cov layout");
static_assert(sizeof(RigCamRec) == sizeof(asl_rig_camera) && sizeof(asl_rig_camera) == 216, "asl_rig_camera layout");
static_assert(sizeof(CalibResultRec) == sizeof(asl_calib_result) && sizeof(asl_calib_result) == 216, "asl_calib_result layout");
static_assert(sizeof(MapResultRec) == sizeof(asl_map_result) && sizeof(asl_map_result) == 64, "asl_map_result layout");
static_assert(sizeof(SmoothResultRec) == sizeof(asl_smooth_result) && sizeof(asl_smooth_result) == 64, "asl_smooth_result layout");

// The camera model as the entry points take it (K and dist are host arrays).  K NULL is each solver's "NULL argument".
struct Camera {
    const double *K, *dist; int n_dist; double tag_size;
};

// solved: calibration, which takes the number of coefficients to solve for and no dist
static int check_camera(const Camera &c, bool solved = false)
{
    if (int rc = check_n_dist(c.n_dist)) return rc;
    if (c.n_dist && !c.dist && !solved) return fail(ASL_EINVAL, "dist is NULL with n_dist = %d", c.n_dist);
    if (!(c.tag_size > 0) || !std::isfinite(c.tag_size)) return fail(ASL_EINVAL, "tag_size must be positive (got %g)", c.tag_size);
    return ASL_OK;
}

static CamDev make_cam(const asl_detector *d, const Camera &c) { return make_cam(d, c.K, c.dist, c.n_dist, c.tag_size); }

// The checks the solvers share on the obs block (max_tags slots per frame, ids below n_ids) and the camera
static int check_obs_args(int max_tags, int n_ids, const Camera &cam, bool solved = false)
{
    if (max_tags < 1 || max_tags > 256) return fail(ASL_EINVAL, "max_tags must be in [1, 256] (got %d)", max_tags);
    if (n_ids < 1) return fail(ASL_EINVAL, "n_ids must be >= 1 (got %d)", n_ids);
    return check_camera(cam, solved);
}

static int check_sigma_px(double sigma_px)
{
    if (!(sigma_px >= 0) || !std::isfinite(sigma_px)) return fail(ASL_EINVAL, "sigma_px must be >= 0 and finite (got %g)", sigma_px);
    return ASL_OK;
}

// The device forms: every refusal, then the launch on the caller's stream
template <class Call, int (*check)(const asl_detector *, const Call &, bool), int (*launch)(asl_detector *, const Call &, hipStream_t)>
static int frames_device(asl_detector *d, const Call &c, void *stream)
{
    if (int rc = check(d, c, true)) return rc;
    HIPCHK(hipSetDevice(d->device));
    return launch(d, c, (hipStream_t)stream);
}

// One piece of d->solve_out in a host (*_batch) form: a result the kernels write at dev and fetch_out copies to host.  No
// bytes: an output the caller did not ask for, dev stays NULL.  host NULL: staged on the device only (smoothing's seed).
struct OutPiece {
    void *host; size_t bytes; void *dev;
};

// The host forms begin here: the pieces carved from solve_out, the host obs block (rows x max_tags) and the map, if given
// (n_maps tables of n_ids entries: the bundle forms have more than one), into the detector's device copies
template <size_t N>
static int stage_host_call(asl_detector *d, const char *what, OutPiece (&pieces)[N], const void *obs, int rows, int max_tags, const void *map, int n_ids,
                           size_t n_maps = 1)
{
    HIPCHK(hipSetDevice(d->device));
    const size_t obs_bytes = sizeof(asl_obs) * (size_t)rows * (size_t)max_tags, map_bytes = sizeof(asl_map_tag) * (size_t)n_ids * n_maps;
    if (carve_ws(d->solve_out, [&](WsCarve &w) { for (OutPiece &p : pieces) p.dev = p.bytes ? w.take<uint8_t>(p.bytes) : nullptr; }) ||
        d->loc_obs.ensure(obs_bytes) || (map && d->loc_map.ensure(map_bytes)))
        return fail(ASL_ENOMEM, "%s workspace allocation failed", what);
    HIPCHK(hipMemcpy(d->loc_obs.p, obs, obs_bytes, hipMemcpyHostToDevice));
    if (map) HIPCHK(hipMemcpy(d->loc_map.p, map, map_bytes, hipMemcpyHostToDevice));
    return ASL_OK;
}

// and end here: the results back
template <size_t N>
static int fetch_out(const OutPiece (&pieces)[N])
{
    for (const OutPiece &p : pieces)
        if (p.host && p.bytes) HIPCHK(hipMemcpy(p.host, p.dev, p.bytes, hipMemcpyDeviceToHost));
    return ASL_OK;
}

// ---- localisation of single frames, one camera or a rig (k_localize.inc, k_rig.inc)

// one camera table, wherever it came from: the model and the mounting of every camera
static int check_rig_table(const asl_rig_camera *rig, int n_cams)
{
    for (int c = 0; c < n_cams; c++) {
        const asl_rig_camera &r = rig[c];
        if (check_n_dist(r.n_dist)) return fail(ASL_EINVAL, "camera %d: n_dist must be 0, 4 or 5 (got %d)", c, r.n_dist);
        for (int k = 0; k < 9; k++)
            if (!std::isfinite(r.K[k])) return fail(ASL_EINVAL, "camera %d: K is not finite", c);
        for (int k = 0; k < r.n_dist; k++)
            if (!std::isfinite(r.dist[k])) return fail(ASL_EINVAL, "camera %d: dist is not finite", c);
        for (int k = 0; k < 12; k++)
            if (!std::isfinite(r.E[k])) return fail(ASL_EINVAL, "camera %d: E is not finite", c);
        const double *E = r.E;
        double dev = 0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                dev = std::max(dev, std::fabs(E[4 * i] * E[4 * j] + E[4 * i + 1] * E[4 * j + 1] + E[4 * i + 2] * E[4 * j + 2] - (i == j ? 1.0 : 0.0)));
        const double det = E[0] * (E[5] * E[10] - E[6] * E[9]) - E[1] * (E[4] * E[10] - E[6] * E[8]) + E[2] * (E[4] * E[9] - E[5] * E[8]);
        if (!(dev <= 1e-6) || !(det > 0))
            return fail(ASL_EINVAL, "camera %d: the rotation part of E is not a rotation (|R R^T - I| = %g, det %g)", c, dev, det);
    }
    return ASL_OK;
}

// One localisation call, whichever of the twelve entry points made it, in their argument order.  The single-camera forms
// leave n_cams 0 and rig NULL; the rig forms give n_cams and the table and leave cam's K and dist NULL, n_dist 0.
// The plain forms leave sigma_px 0 and cov NULL.  obs, map, rig, out and cov are all host or all device pointers.
struct LocCall {
    const void *obs; int n_cams, n_frames, max_tags;
    const void *map; int n_ids;
    const void *rig; Camera cam;
    double gate, sigma_px;
    void *out, *cov;
    bool with_cov;      // a covariance form: cov must be there
    // the mapcov forms (asl_localize_mapcov_*, asl_localize_rig_mapcov_*): the map's joint covariance as asl_mapcov_* writes
    // it, host or device as the rest; every other form leaves them NULL, 0 and false
    const void *map_cov; int ld; const void *cov_slot;
    bool with_mapcov;
    // the bundle forms (asl_localize_bundles_*): map is n_bundles tables of n_ids entries (bundle<-tag), out and cov
    // n_frames x n_bundles records; every other form leaves it 0, which is one table and one record per frame
    int n_bundles;
    bool with_bundles;
};

#define LOC_MAX_BUNDLES 1024

static bool is_rig(const LocCall &c) { return c.n_cams || c.rig; }

// The mapcov host forms' look at what the device forms can only report through asl_pose_cov.status 3: every cov_slot entry
// in [-1, ld / 6), and every entry of the blocks they refer to finite
static int check_map_cov_host(const int32_t *slot, int n_ids, const double *cov, int ld)
{
    int n = 0;
    for (int i = 0; i < n_ids; i++) {
        if (slot[i] < -1 || slot[i] >= ld / 6) return fail(ASL_EINVAL, "cov_slot[%d] must be in [-1, %d) (got %d)", i, ld / 6, slot[i]);
        n = std::max(n, slot[i] + 1);
    }
    for (int r = 0; r < 6 * n; r++)
        for (int c = 0; c < 6 * n; c++)
            if (!std::isfinite(cov[(size_t)r * ld + c])) return fail(ASL_EINVAL, "map_cov is not finite at (%d, %d)", r, c);
    return ASL_OK;
}

// Every refusal, before anything is written or enqueued.  A rig's table is checked last: where it is, or (device: the
// pointers are the device's) in a copy read back, at most 16 x 216 bytes; it must be complete when the call is made.
static int check_localize_call(const asl_detector *d, const LocCall &c, bool device)
{
    const bool rig = is_rig(c);
    if (c.with_cov && !c.cov) return fail(ASL_EINVAL, "NULL argument");
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.map || !(rig ? c.rig : (const void *)c.cam.K) || !c.out) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_frames < 0) return fail(ASL_EINVAL, "n_frames < 0");
    if (c.with_bundles) {
        if (c.n_bundles < 1 || c.n_bundles > LOC_MAX_BUNDLES)
            return fail(ASL_EINVAL, "n_bundles must be in [1, %d] (got %d)", LOC_MAX_BUNDLES, c.n_bundles);
        if ((long long)c.n_frames * c.n_bundles > INT32_MAX)
            return fail(ASL_EINVAL, "n_frames * n_bundles must fit 32 bits (got %d x %d)", c.n_frames, c.n_bundles);
    }
    if (rig && (c.n_cams < 1 || c.n_cams > RIG_MAX_CAMS)) return fail(ASL_EINVAL, "n_cams must be in [1, %d] (got %d)", RIG_MAX_CAMS, c.n_cams);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, c.cam)) return rc;
    if (rig && c.n_cams * c.max_tags > RIG_MAX_SLOTS)
        return fail(ASL_EINVAL, "n_cams * max_tags must be <= %d (got %d x %d)", RIG_MAX_SLOTS, c.n_cams, c.max_tags);
    if (!(c.gate >= 0) || !std::isfinite(c.gate)) return fail(ASL_EINVAL, "max_tag_rms_px must be >= 0 (got %g)", c.gate);
    if (int rc = check_sigma_px(c.sigma_px)) return rc;
    if (c.with_mapcov) {
        if (!c.map_cov || !c.cov_slot) return fail(ASL_EINVAL, "NULL argument");
        if (c.ld < 6 || c.ld % 6) return fail(ASL_EINVAL, "ld must be a positive multiple of 6 (got %d)", c.ld);
        if (!device)
            if (int rc = check_map_cov_host((const int32_t *)c.cov_slot, c.n_ids, (const double *)c.map_cov, c.ld)) return rc;
    }
    if (!rig) return ASL_OK;
    asl_rig_camera tab[RIG_MAX_CAMS];
    if (device) {
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipMemcpy(tab, c.rig, sizeof(asl_rig_camera) * (size_t)c.n_cams, hipMemcpyDeviceToHost));
    }
    return check_rig_table(device ? tab : (const asl_rig_camera *)c.rig, c.n_cams);
}

// c's pointers are the device's; cov NULL: the plain kernel
static int launch_localize(asl_detector *d, const LocCall &c, hipStream_t st)
{
    if (c.n_frames == 0) return ASL_OK;
    static const double no_K[9] = {};
    const bool rig = is_rig(c);
    const CamDev cam = make_cam(d, rig ? no_K : c.cam.K, c.cam.dist, c.cam.n_dist, c.cam.tag_size);   // a rig: for its half alone
    const dim3 grid((unsigned int)c.n_frames, (unsigned int)std::max(c.n_bundles, 1)), block(ASL_WAVE);   // (frame, bundle)
    const ObsRec *obs = (const ObsRec *)c.obs;
    const MapTagRec *map = (const MapTagRec *)c.map;
    const RigCamRec *tab = (const RigCamRec *)c.rig;
    CamPoseRec *out = (CamPoseRec *)c.out;
    PoseCovRec *cov = (PoseCovRec *)c.cov;
    const size_t lds = rig ? rig_lds_bytes(c.n_cams, c.max_tags) : loc_lds_bytes(c.max_tags);
    const LocMapCov mc{(const double *)c.map_cov, (const int *)c.cov_slot, c.ld};
    if (c.with_mapcov && !rig)
        hipLaunchKernelGGL(k_localize_mapcov, grid, block, lds, st, obs, c.max_tags, map, c.n_ids, cam, c.gate, out, cov, c.sigma_px, mc);
    else if (c.with_mapcov)
        hipLaunchKernelGGL(k_localize_rig_mapcov, grid, block, lds, st, obs, c.n_cams, c.max_tags, map, c.n_ids, tab, cam.half, c.gate, out, cov,
                           c.sigma_px, mc);
    else if (!rig && cov)
        hipLaunchKernelGGL(k_localize<true>, grid, block, lds, st, obs, c.max_tags, map, c.n_ids, cam, c.gate, out, cov, c.sigma_px);
    else if (!rig)
        hipLaunchKernelGGL(k_localize<false>, grid, block, lds, st, obs, c.max_tags, map, c.n_ids, cam, c.gate, out, cov, c.sigma_px);
    else if (cov)
        hipLaunchKernelGGL(k_localize_rig<true>, grid, block, lds, st, obs, c.n_cams, c.max_tags, map, c.n_ids, tab, cam.half, c.gate, out, cov, c.sigma_px);
    else
        hipLaunchKernelGGL(k_localize_rig<false>, grid, block, lds, st, obs, c.n_cams, c.max_tags, map, c.n_ids, tab, cam.half, c.gate, out, cov, c.sigma_px);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static constexpr auto localize_frames_device = frames_device<LocCall, check_localize_call, launch_localize>;   // the four device forms

// the four host forms; a rig's table is staged in solve_out too
static int localize_batch(asl_detector *d, const LocCall &c)
{
    if (int rc = check_localize_call(d, c, false)) return rc;
    if (c.n_frames == 0) return ASL_OK;
    const bool rig = is_rig(c);
    const size_t nb_maps = (size_t)std::max(c.n_bundles, 1);   // the bundle forms: that many tables in, records per frame out
    const size_t n = (size_t)c.n_frames * nb_maps, rig_bytes = sizeof(asl_rig_camera) * (size_t)c.n_cams;
    // the mapcov forms: the blocks the slots refer to (the leading 6 n x 6 n region) staged with 6 n as the leading dimension
    size_t nb = 0;
    for (int i = 0; c.with_mapcov && i < c.n_ids; i++) nb = std::max(nb, (size_t)(((const int32_t *)c.cov_slot)[i] + 1));
    const size_t ldd = 6 * std::max<size_t>(nb, 1), slot_bytes = c.with_mapcov ? sizeof(int32_t) * (size_t)c.n_ids : 0;
    OutPiece o[] = {{c.out, sizeof(asl_cam_pose) * n}, {c.cov, c.cov ? sizeof(asl_pose_cov) * n : 0}, {nullptr, rig_bytes}, {nullptr, slot_bytes},
                    {nullptr, c.with_mapcov ? sizeof(double) * ldd * ldd : 0}};
    if (int rc = stage_host_call(d, rig ? "rig localisation" : "localisation", o, c.obs, (rig ? c.n_cams : 1) * c.n_frames, c.max_tags, c.map, c.n_ids,
                                 nb_maps))
        return rc;
    if (rig) HIPCHK(hipMemcpy(o[2].dev, c.rig, rig_bytes, hipMemcpyHostToDevice));
    LocCall dc = c;
    dc.obs = d->loc_obs.p; dc.map = d->loc_map.p; dc.out = o[0].dev; dc.cov = o[1].dev; dc.rig = o[2].dev;
    if (c.with_mapcov) {
        HIPCHK(hipMemcpy(o[3].dev, c.cov_slot, slot_bytes, hipMemcpyHostToDevice));
        if (nb)
            HIPCHK(hipMemcpy2D(o[4].dev, sizeof(double) * ldd, c.map_cov, sizeof(double) * (size_t)c.ld, sizeof(double) * 6 * nb, 6 * nb,
                               hipMemcpyHostToDevice));
        dc.cov_slot = o[3].dev; dc.map_cov = o[4].dev; dc.ld = (int)ldd;
    }
    if (int rc = launch_localize(d, dc, nullptr)) return rc;
    return fetch_out(o);
}

extern "C" int asl_localize_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                          const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                          void *d_out, void *stream)
{
    return localize_frames_device(d, {d_obs, 0, n_frames, max_tags, d_map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, 0.0, d_out, nullptr, false}, stream);
}

extern "C" int asl_localize_cov_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                              const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                              double sigma_px, void *d_out, void *d_cov, void *stream)
{
    return localize_frames_device(d, {d_obs, 0, n_frames, max_tags, d_map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, d_out, d_cov, true}, stream);
}

extern "C" int asl_localize_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                  const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px, asl_cam_pose *out)
{
    return localize_batch(d, {obs, 0, n_frames, max_tags, map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, 0.0, out, nullptr, false});
}

extern "C" int asl_localize_cov_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                      const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px, double sigma_px,
                                      asl_cam_pose *out, asl_pose_cov *cov)
{
    return localize_batch(d, {obs, 0, n_frames, max_tags, map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, out, cov, true});
}

extern "C" int asl_localize_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                              int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px, void *d_out, void *stream)
{
    return localize_frames_device(d, {d_obs, n_cams, n_frames, max_tags, d_map, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, 0.0, d_out, nullptr, false}, stream);
}

extern "C" int asl_localize_rig_cov_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                                  int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                                  void *d_out, void *d_cov, void *stream)
{
    return localize_frames_device(d, {d_obs, n_cams, n_frames, max_tags, d_map, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, d_out, d_cov, true}, stream);
}

extern "C" int asl_localize_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                      const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, asl_cam_pose *out)
{
    return localize_batch(d, {obs, n_cams, n_frames, max_tags, map, n_ids, rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, 0.0, out, nullptr, false});
}

extern "C" int asl_localize_rig_cov_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                                          int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                          asl_cam_pose *out, asl_pose_cov *cov)
{
    return localize_batch(d, {obs, n_cams, n_frames, max_tags, map, n_ids, rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, out, cov, true});
}

// The mapcov forms: the _cov argument lists with the map's joint covariance (map_cov, ld, cov_slot) after cov.
extern "C" int asl_localize_mapcov_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                                 const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                                 double sigma_px, void *d_out, void *d_cov, const void *d_map_cov, int ld, const void *d_cov_slot,
                                                 void *stream)
{
    return localize_frames_device(d, {d_obs, 0, n_frames, max_tags, d_map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, d_out, d_cov, true,
                                      d_map_cov, ld, d_cov_slot, true}, stream);
}

extern "C" int asl_localize_mapcov_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                         const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px, double sigma_px,
                                         asl_cam_pose *out, asl_pose_cov *cov, const double *map_cov, int ld, const int32_t *cov_slot)
{
    return localize_batch(d, {obs, 0, n_frames, max_tags, map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, out, cov, true,
                              map_cov, ld, cov_slot, true});
}

extern "C" int asl_localize_rig_mapcov_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                                     int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                                     void *d_out, void *d_cov, const void *d_map_cov, int ld, const void *d_cov_slot, void *stream)
{
    return localize_frames_device(d, {d_obs, n_cams, n_frames, max_tags, d_map, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, d_out,
                                      d_cov, true, d_map_cov, ld, d_cov_slot, true}, stream);
}

extern "C" int asl_localize_rig_mapcov_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                                             int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                             asl_cam_pose *out, asl_pose_cov *cov, const double *map_cov, int ld, const int32_t *cov_slot)
{
    return localize_batch(d, {obs, n_cams, n_frames, max_tags, map, n_ids, rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, out, cov, true,
                              map_cov, ld, cov_slot, true});
}

// The bundle forms: the one-map argument lists with n_bundles after the tables, and d_cov NULL (cov NULL) for the plain kernel.
extern "C" int asl_localize_bundles_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_maps, int n_bundles,
                                                  int n_ids, const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                                  double sigma_px, void *d_out, void *d_cov, void *stream)
{
    return localize_frames_device(d, {d_obs, 0, n_frames, max_tags, d_maps, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, d_out, d_cov,
                                      false, nullptr, 0, nullptr, false, n_bundles, true}, stream);
}

extern "C" int asl_localize_bundles_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *maps, int n_bundles,
                                          int n_ids, const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                          double sigma_px, asl_cam_pose *out, asl_pose_cov *cov)
{
    return localize_batch(d, {obs, 0, n_frames, max_tags, maps, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_tag_rms_px, sigma_px, out, cov, false,
                              nullptr, 0, nullptr, false, n_bundles, true});
}

extern "C" int asl_localize_bundles_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_maps,
                                                      int n_bundles, int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px,
                                                      double sigma_px, void *d_out, void *d_cov, void *stream)
{
    return localize_frames_device(d, {d_obs, n_cams, n_frames, max_tags, d_maps, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, d_out,
                                      d_cov, false, nullptr, 0, nullptr, false, n_bundles, true}, stream);
}

extern "C" int asl_localize_bundles_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *maps,
                                              int n_bundles, int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px,
                                              double sigma_px, asl_cam_pose *out, asl_pose_cov *cov)
{
    return localize_batch(d, {obs, n_cams, n_frames, max_tags, maps, n_ids, rig, {nullptr, nullptr, 0, tag_size}, max_tag_rms_px, sigma_px, out, cov, false,
                              nullptr, 0, nullptr, false, n_bundles, true});
}

// ---- the pose of one bundle in another's frame (k_bundle.inc)

static_assert(sizeof(BundleRelRec) == sizeof(asl_bundle_rel) && sizeof(asl_bundle_rel) == 424, "asl_bundle_rel layout");

// n_frames x n_bundles poses, and their covariances or NULL -> as many asl_bundle_rel; all host or all device pointers
struct BundleRelCall {
    const void *poses, *cov; int n_frames, n_bundles, ref;
    void *rel;
};

static int check_bundle_rel_call(const asl_detector *d, const BundleRelCall &c, bool)
{
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.poses || !c.rel) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_frames < 0) return fail(ASL_EINVAL, "n_frames < 0");
    if (c.n_bundles < 1 || c.n_bundles > LOC_MAX_BUNDLES) return fail(ASL_EINVAL, "n_bundles must be in [1, %d] (got %d)", LOC_MAX_BUNDLES, c.n_bundles);
    if ((long long)c.n_frames * c.n_bundles > INT32_MAX)
        return fail(ASL_EINVAL, "n_frames * n_bundles must fit 32 bits (got %d x %d)", c.n_frames, c.n_bundles);
    if (c.ref < 0 || c.ref >= c.n_bundles) return fail(ASL_EINVAL, "ref must be in [0, %d) (got %d)", c.n_bundles, c.ref);
    return ASL_OK;
}

static int launch_bundle_rel(asl_detector *, const BundleRelCall &c, hipStream_t st)
{
    const long long n = (long long)c.n_frames * c.n_bundles;
    if (n == 0) return ASL_OK;
    hipLaunchKernelGGL(k_bundle_relative, dim3((unsigned int)((n + ASL_WAVE - 1) / ASL_WAVE)), dim3(ASL_WAVE), 0, st, (const CamPoseRec *)c.poses,
                       (const PoseCovRec *)c.cov, c.n_frames, c.n_bundles, c.ref, (BundleRelRec *)c.rel);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_bundle_relative_device(asl_detector *d, const void *d_poses, const void *d_cov, int n_frames, int n_bundles, int ref, void *d_rel,
                                          void *stream)
{
    return frames_device<BundleRelCall, check_bundle_rel_call, launch_bundle_rel>(d, {d_poses, d_cov, n_frames, n_bundles, ref, d_rel}, stream);
}

extern "C" int asl_bundle_relative_batch(asl_detector *d, const asl_cam_pose *poses, const asl_pose_cov *cov, int n_frames, int n_bundles, int ref,
                                         asl_bundle_rel *rel)
{
    const BundleRelCall c{poses, cov, n_frames, n_bundles, ref, rel};
    if (int rc = check_bundle_rel_call(d, c, false)) return rc;
    const size_t n = (size_t)n_frames * (size_t)n_bundles;
    if (n == 0) return ASL_OK;
    HIPCHK(hipSetDevice(d->device));
    // the poses and covariances in, staged in solve_out beside the result
    OutPiece o[] = {{rel, sizeof(asl_bundle_rel) * n}, {nullptr, sizeof(asl_cam_pose) * n}, {nullptr, cov ? sizeof(asl_pose_cov) * n : 0}};
    if (carve_ws(d->solve_out, [&](WsCarve &w) { for (OutPiece &p : o) p.dev = p.bytes ? w.take<uint8_t>(p.bytes) : nullptr; }))
        return fail(ASL_ENOMEM, "bundle workspace allocation failed");
    HIPCHK(hipMemcpy(o[1].dev, poses, o[1].bytes, hipMemcpyHostToDevice));
    if (cov) HIPCHK(hipMemcpy(o[2].dev, cov, o[2].bytes, hipMemcpyHostToDevice));
    if (int rc = launch_bundle_rel(d, {o[1].dev, o[2].dev, n_frames, n_bundles, ref, o[0].dev}, nullptr)) return rc;
    return fetch_out(o);
}

// ---- per-tag pose covariance (k_posecov.inc)

// n asl_obs records with their poses -> n asl_pose_cov; obs and cov are both host or both device pointers
struct PoseCovCall {
    const void *obs; int n;
    Camera cam; double sigma_px;
    void *cov;
};

static int check_pose_cov_call(const asl_detector *d, const PoseCovCall &c, bool)
{
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.cam.K || !c.cov) return fail(ASL_EINVAL, "NULL argument");
    if (c.n < 0) return fail(ASL_EINVAL, "record count < 0");
    if (int rc = check_camera(c.cam)) return rc;
    return check_sigma_px(c.sigma_px);
}

static int launch_pose_cov(asl_detector *d, const PoseCovCall &c, hipStream_t st)
{
    if (c.n == 0) return ASL_OK;
    hipLaunchKernelGGL(k_pnp_cov, dim3((unsigned int)((c.n + PNP_TAGS_PER_WAVE - 1) / PNP_TAGS_PER_WAVE)), dim3(ASL_WAVE), 0, st, (const ObsRec *)c.obs, c.n,
                       make_cam(d, c.cam), c.sigma_px, (PoseCovRec *)c.cov);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

extern "C" int asl_pose_cov_device(asl_detector *d, const void *d_obs, int n_records, const double *K, const double *dist, int n_dist,
                                   double tag_size, double sigma_px, void *d_cov, void *stream)
{
    return frames_device<PoseCovCall, check_pose_cov_call, launch_pose_cov>(d, {d_obs, n_records, {K, dist, n_dist, tag_size}, sigma_px, d_cov}, stream);
}

extern "C" int asl_solve_pnp_cov_batch(asl_detector *d, const float *corners, const double *T, const double *K, const double *dist, int n_dist,
                                       double tag_size, double sigma_px, asl_pose_cov *cov, int N)
{
    // the records are made of corners and T: either missing is the missing obs
    if (int rc = check_pose_cov_call(d, {T ? corners : nullptr, N, {K, dist, n_dist, tag_size}, sigma_px, cov}, false)) return rc;
    if (N == 0) return ASL_OK;
    std::vector<asl_obs> rec((size_t)N);
    for (int i = 0; i < N; i++) {  // a pose with a non-finite entry (a failed PnP) is no pose: status 1
        bool finite = true;
        for (int k = 0; k < 12; k++) finite = finite && std::isfinite(T[16 * (size_t)i + k]);
        rec[i].id = 0; rec[i].flags = finite ? 3 : 1;
        memcpy(rec[i].corners, corners + 8 * (size_t)i, sizeof rec[i].corners);
        memcpy(rec[i].T, T + 16 * (size_t)i, sizeof rec[i].T);
    }
    OutPiece o[] = {{cov, sizeof(asl_pose_cov) * (size_t)N}};
    if (int rc = stage_host_call(d, "pose covariance", o, rec.data(), 1, N, nullptr, 0)) return rc;
    if (int rc = launch_pose_cov(d, {d->loc_obs.p, N, {K, dist, n_dist, tag_size}, sigma_px, o[0].dev}, nullptr)) return rc;
    return fetch_out(o);
}

// ---- calibration (k_calib.inc)

// One calibration call, in the entry points' argument order; K_init may be NULL.  obs, map, result and poses are all host
// (asl_calibrate_batch, asl_calibrate_lens_batch) or all device pointers (the *_frames_device forms); no field is left empty
// by either.  lens_model comes last here: the asl_calibrate_* forms leave it out, which is ASL_LENS_BROWN.
struct CalibCall {
    const void *obs; int n_frames, max_tags;
    const void *map; int n_ids;
    double tag_size; int width, height;
    const double *K_init; int n_dist, flags, max_iters;
    void *result, *poses;
    int lens_model;
};

// every refusal, before anything is written or enqueued; the same for both forms
static int check_calibrate_call(const asl_detector *d, const CalibCall &c, bool)
{
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.map || !c.result || !c.poses) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_frames < 1) return fail(ASL_EINVAL, "n_frames must be >= 1 (got %d)", c.n_frames);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, {nullptr, nullptr, c.n_dist, c.tag_size}, true)) return rc;
    if (c.width < 1 || c.height < 1) return fail(ASL_EINVAL, "width and height must be positive (got %d x %d)", c.width, c.height);
    if (c.max_iters < 1) return fail(ASL_EINVAL, "max_iters must be >= 1 (got %d)", c.max_iters);
    if (c.flags & ~(ASL_CALIB_FIX_PRINCIPAL_POINT | ASL_CALIB_FIX_ASPECT_RATIO | ASL_CALIB_ZERO_TANGENT_DIST))
        return fail(ASL_EINVAL, "unknown calibration flags 0x%x", c.flags);
    if (c.lens_model != ASL_LENS_BROWN && c.lens_model != ASL_LENS_FISHEYE) return fail(ASL_EINVAL, "lens_model must be 0 or 1 (got %d)", c.lens_model);
    if (c.lens_model == ASL_LENS_FISHEYE) {
        if (c.n_dist != 0 && c.n_dist != 4) return fail(ASL_EINVAL, "a fisheye lens has 0 or 4 coefficients (got n_dist = %d)", c.n_dist);
        if (c.flags & ASL_CALIB_ZERO_TANGENT_DIST) return fail(ASL_EINVAL, "ASL_CALIB_ZERO_TANGENT_DIST has no meaning under the fisheye lens");
    }
    if (const double *K = c.K_init; K && !(K[0] > 0 && K[4] > 0 && std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) && std::isfinite(K[5])))
        return fail(ASL_EINVAL, "K_init must have finite, positive focal lengths");
    return ASL_OK;
}

// c's pointers are the device's.  The calibration workspace: state, frame lists and per-frame buffers, carved from d->cal_ws
static int launch_calibrate(asl_detector *d, const CalibCall &c, hipStream_t st)
{
    const size_t nf = (size_t)c.n_frames;
    const bool fisheye = c.lens_model == ASL_LENS_FISHEYE;
    CalibArgs a{};
    a.lens = fisheye ? CAL_LENS_FISHEYE : CAL_LENS_BROWN;
    a.n_rungs = fisheye ? (c.K_init ? 1 : CAL_RUNGS) : 0;  // the ladder's room: none under the Brown lens
    const size_t nl = nf * (size_t)a.n_rungs;
    if (carve_ws(d->cal_ws, [&](WsCarve &w) {
            a.st = w.take<CalibState>(1); a.list = w.take<int>(nf); a.fr = w.take<int>(CAL_FR * nf);
            a.zh = w.take<double>(CAL_ZH * nf); a.seedc = w.take<double>(nf); a.pose = w.take<double>(2 * 12 * nf);
            a.H = w.take<double>(2 * CAL_HS * nf); a.SB = w.take<double>(CAL_SB * nf); a.back = w.take<double>(CAL_BK * nf);
            a.lpose = w.take<double>(12 * nl); a.lcost = w.take<double>(nl); a.lcode = w.take<int>(nl);
        }))
        return fail(ASL_ENOMEM, "calibration workspace allocation failed");
    a.obs = (const ObsRec *)c.obs; a.map = (const MapTagRec *)c.map;
    a.res = (CalibResultRec *)c.result; a.out = (CamPoseRec *)c.poses;
    a.half = (double)(float)(c.tag_size / 2);  // object corners are float32, as in the PnP
    a.width = c.width; a.height = c.height;
    a.has_init = c.K_init != nullptr;
    if (c.K_init) { a.Kinit[0] = c.K_init[0]; a.Kinit[1] = c.K_init[4]; a.Kinit[2] = c.K_init[2]; a.Kinit[3] = c.K_init[5]; }
    a.n_frames = c.n_frames; a.max_tags = c.max_tags; a.n_ids = c.n_ids; a.n_dist = c.n_dist; a.flags = c.flags; a.max_iters = c.max_iters;
    int np = 0;  // the free entries of (fx, fy, cx, cy, k1, k2, p1, p2, k3); a fisheye: (.., k1, k2, k3, k4), all four free
    if (!(c.flags & ASL_CALIB_FIX_ASPECT_RATIO)) a.sel[np++] = 0;
    a.sel[np++] = 1;
    if (!(c.flags & ASL_CALIB_FIX_PRINCIPAL_POINT)) { a.sel[np++] = 2; a.sel[np++] = 3; }
    if (c.n_dist >= 4) {
        a.sel[np++] = 4; a.sel[np++] = 5;
        if (!(c.flags & ASL_CALIB_ZERO_TANGENT_DIST)) { a.sel[np++] = 6; a.sel[np++] = 7; }
    }
    if (c.n_dist == 5) a.sel[np++] = 8;
    a.np = np;
    const dim3 frames((unsigned int)c.n_frames), wave(ASL_WAVE), wg(CAL_WG);
    const size_t lds = loc_lds_bytes(c.max_tags);
    auto seed = c.n_dist == 5 ? k_calib_seed<5> : c.n_dist == 4 ? k_calib_seed<4> : k_calib_seed<0>;
    auto step = c.n_dist == 5 ? k_calib_step<5> : c.n_dist == 4 ? k_calib_step<4> : k_calib_step<0>;
    if (fisheye) step = c.n_dist == 4 ? k_calib_step<4, CAL_LENS_FISHEYE> : k_calib_step<0, CAL_LENS_FISHEYE>;
    hipLaunchKernelGGL(k_calib_init, frames, wave, 0, st, a);
    hipLaunchKernelGGL(k_calib_k0, dim3(1), wg, 0, st, a);
    if (fisheye) {
        hipLaunchKernelGGL(k_calib_fish_seed, dim3((unsigned int)c.n_frames, (unsigned int)a.n_rungs), wave, lds, st, a);
        hipLaunchKernelGGL(k_calib_fish_pick, dim3(1), wg, 0, st, a);
        hipLaunchKernelGGL(c.n_dist == 4 ? k_calib_fish_lin<4> : k_calib_fish_lin<0>, frames, wave, lds, st, a);
    } else
        hipLaunchKernelGGL(seed, frames, wave, lds, st, a);
    hipLaunchKernelGGL(k_calib_start, dim3(1), wg, 0, st, a);
    for (int it = 0; it < c.max_iters; it++) {
        hipLaunchKernelGGL(k_calib_schur, frames, wave, 0, st, a, 0);
        hipLaunchKernelGGL(k_calib_solve, dim3(1), wg, 0, st, a);
        hipLaunchKernelGGL(step, frames, wave, lds, st, a);
        hipLaunchKernelGGL(k_calib_decide, dim3(1), wg, 0, st, a);
    }
    hipLaunchKernelGGL(k_calib_schur, frames, wave, 0, st, a, 1);
    hipLaunchKernelGGL(k_calib_finish, dim3(1), wg, 0, st, a);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static constexpr auto calibrate_frames_device = frames_device<CalibCall, check_calibrate_call, launch_calibrate>;

static int calibrate_batch(asl_detector *d, const CalibCall &c)
{
    if (int rc = check_calibrate_call(d, c, false)) return rc;
    OutPiece o[] = {{c.result, sizeof(asl_calib_result)}, {c.poses, sizeof(asl_cam_pose) * (size_t)c.n_frames}};
    if (int rc = stage_host_call(d, "calibration", o, c.obs, c.n_frames, c.max_tags, c.map, c.n_ids)) return rc;
    CalibCall dc = c;
    dc.obs = d->loc_obs.p; dc.map = d->loc_map.p; dc.result = o[0].dev; dc.poses = o[1].dev;
    if (int rc = launch_calibrate(d, dc, nullptr)) return rc;
    return fetch_out(o);
}

extern "C" int asl_calibrate_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                           double tag_size, int width, int height, const double *K_init, int n_dist, int flags, int max_iters,
                                           void *d_result, void *d_poses, void *stream)
{
    return calibrate_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, tag_size, width, height, K_init, n_dist, flags, max_iters, d_result, d_poses}, stream);
}

extern "C" int asl_calibrate_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                   double tag_size, int width, int height, const double *K_init, int n_dist, int flags, int max_iters,
                                   asl_calib_result *result, asl_cam_pose *poses)
{
    return calibrate_batch(d, {obs, n_frames, max_tags, map, n_ids, tag_size, width, height, K_init, n_dist, flags, max_iters, result, poses});
}

// the same call records with the lens named: ASL_LENS_BROWN is the two entry points above
extern "C" int asl_calibrate_lens_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                                double tag_size, int width, int height, const double *K_init, int lens_model, int n_dist, int flags,
                                                int max_iters, void *d_result, void *d_poses, void *stream)
{
    return calibrate_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, tag_size, width, height, K_init, n_dist, flags, max_iters, d_result, d_poses, lens_model},
                                   stream);
}

extern "C" int asl_calibrate_lens_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                        double tag_size, int width, int height, const double *K_init, int lens_model, int n_dist, int flags,
                                        int max_iters, asl_calib_result *result, asl_cam_pose *poses)
{
    return calibrate_batch(d, {obs, n_frames, max_tags, map, n_ids, tag_size, width, height, K_init, n_dist, flags, max_iters, result, poses, lens_model});
}

// ---- rig mounting calibration (k_rigcal.inc)

static_assert(sizeof(RigCalResultRec) == sizeof(asl_rig_calib_result) && sizeof(asl_rig_calib_result) == 176, "asl_rig_calib_result layout");

// One mounting calibration call, in the entry points' argument order.  obs, map, rig, rig_out, result, cov and poses are all
// host (asl_calibrate_rig_batch) or all device pointers (asl_calibrate_rig_frames_device); rig_out may be rig.
struct RigCalCall {
    const void *obs; int n_cams, n_frames, max_tags;
    const void *map; int n_ids;
    const void *rig; double tag_size; int max_iters; double sigma_px;
    void *rig_out, *result, *cov, *poses;
};

// every refusal, before anything is written or enqueued; the table last, as check_localize_call reads it
static int check_rig_calibrate_call(const asl_detector *d, const RigCalCall &c, bool device)
{
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.map || !c.rig || !c.rig_out || !c.result || !c.cov || !c.poses) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_cams < 2 || c.n_cams > RC_MAX_CAMS) return fail(ASL_EINVAL, "n_cams must be in [2, %d] (got %d)", RC_MAX_CAMS, c.n_cams);
    if (c.n_frames < 1) return fail(ASL_EINVAL, "n_frames must be >= 1 (got %d)", c.n_frames);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, {nullptr, nullptr, 0, c.tag_size})) return rc;
    if (c.n_cams * c.max_tags > RIG_MAX_SLOTS)
        return fail(ASL_EINVAL, "n_cams * max_tags must be <= %d (got %d x %d)", RIG_MAX_SLOTS, c.n_cams, c.max_tags);
    if (c.max_iters < 1) return fail(ASL_EINVAL, "max_iters must be >= 1 (got %d)", c.max_iters);
    if (int rc = check_sigma_px(c.sigma_px)) return rc;
    asl_rig_camera tab[RC_MAX_CAMS];
    if (device) {
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipMemcpy(tab, c.rig, sizeof(asl_rig_camera) * (size_t)c.n_cams, hipMemcpyDeviceToHost));
    }
    return check_rig_table(device ? tab : (const asl_rig_camera *)c.rig, c.n_cams);
}

// c's pointers are the device's.  The workspace: state, frame list and per-frame buffers, carved from d->rigcal_ws
static int launch_rig_calibrate(asl_detector *d, const RigCalCall &c, hipStream_t st)
{
    const size_t nf = (size_t)c.n_frames;
    const int ns = c.n_cams - 1;  // room for every camera but the reference to be solved
    RigCalArgs a{};
    a.hs = rc_hs(ns); a.sbs = rc_sb(ns); a.bks = rc_bk(ns);
    if (carve_ws(d->rigcal_ws, [&](WsCarve &w) {
            a.st = w.take<RigCalState>(1); a.list = w.take<int>(nf); a.fr = w.take<int>(RC_FR * nf);
            a.camtab = w.take<double>(2 * (size_t)c.n_cams * RIG_CAM_DOUBLES); a.pose = w.take<double>(2 * 12 * nf);
            a.H = w.take<double>(2 * (size_t)a.hs * nf); a.SB = w.take<double>((size_t)a.sbs * nf); a.back = w.take<double>((size_t)a.bks * nf);
        }))
        return fail(ASL_ENOMEM, "rig calibration workspace allocation failed");
    a.obs = (const ObsRec *)c.obs; a.map = (const MapTagRec *)c.map;
    a.rig = (const RigCamRec *)c.rig; a.rig_out = (RigCamRec *)c.rig_out;
    a.res = (RigCalResultRec *)c.result; a.cov = (PoseCovRec *)c.cov; a.out = (CamPoseRec *)c.poses;
    a.half = (double)(float)(c.tag_size / 2);  // object corners are float32, as in the PnP
    a.sigma_px = c.sigma_px;
    a.magic = 65536u / (unsigned int)c.max_tags + 1u;
    a.n_cams = c.n_cams; a.n_frames = c.n_frames; a.max_tags = c.max_tags; a.n_ids = c.n_ids; a.max_iters = c.max_iters;
    const dim3 frames((unsigned int)c.n_frames), wave(ASL_WAVE), wg(CAL_WG);
    const size_t lds = rig_lds_bytes(c.n_cams, c.max_tags);
    // the seed: asl_localize_rig_frames_device under the mountings as given, the gate off
    hipLaunchKernelGGL(k_localize_rig<false>, frames, wave, lds, st, a.obs, c.n_cams, c.max_tags, a.map, c.n_ids, a.rig, a.half, 0.0, a.out,
                       (PoseCovRec *)nullptr, 0.0);
    hipLaunchKernelGGL(k_rigcal_init, frames, wave, 0, st, a);
    hipLaunchKernelGGL(k_rigcal_connect, dim3(1), wg, 0, st, a);
    hipLaunchKernelGGL(k_rigcal_first, frames, wave, lds, st, a);
    hipLaunchKernelGGL(k_rigcal_start, dim3(1), wg, 0, st, a);
    for (int it = 0; it < c.max_iters; it++) {
        hipLaunchKernelGGL(k_rigcal_schur, frames, wave, 0, st, a, 0);
        hipLaunchKernelGGL(k_rigcal_solve, dim3(1), wg, 0, st, a);
        hipLaunchKernelGGL(k_rigcal_step, frames, wave, lds, st, a);
        hipLaunchKernelGGL(k_rigcal_decide, dim3(1), wg, 0, st, a);
    }
    hipLaunchKernelGGL(k_rigcal_schur, frames, wave, 0, st, a, 1);
    hipLaunchKernelGGL(k_rigcal_finish, dim3(1), wg, 0, st, a);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static int rig_calibrate_batch(asl_detector *d, const RigCalCall &c)
{
    if (int rc = check_rig_calibrate_call(d, c, false)) return rc;
    const size_t rig_bytes = sizeof(asl_rig_camera) * (size_t)c.n_cams;
    OutPiece o[] = {{c.rig_out, rig_bytes}, {c.result, sizeof(asl_rig_calib_result)}, {c.cov, sizeof(asl_pose_cov) * (size_t)c.n_cams},
                    {c.poses, sizeof(asl_cam_pose) * (size_t)c.n_frames}, {nullptr, rig_bytes}};
    if (int rc = stage_host_call(d, "rig calibration", o, c.obs, c.n_cams * c.n_frames, c.max_tags, c.map, c.n_ids)) return rc;
    HIPCHK(hipMemcpy(o[4].dev, c.rig, rig_bytes, hipMemcpyHostToDevice));
    RigCalCall dc = c;
    dc.obs = d->loc_obs.p; dc.map = d->loc_map.p; dc.rig = o[4].dev;
    dc.rig_out = o[0].dev; dc.result = o[1].dev; dc.cov = o[2].dev; dc.poses = o[3].dev;
    if (int rc = launch_rig_calibrate(d, dc, nullptr)) return rc;
    return fetch_out(o);
}

extern "C" int asl_calibrate_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                               int n_ids, const void *d_rig, double tag_size, int max_iters, double sigma_px, void *d_rig_out,
                                               void *d_result, void *d_cov, void *d_poses, void *stream)
{
    return frames_device<RigCalCall, check_rig_calibrate_call, launch_rig_calibrate>(
        d, {d_obs, n_cams, n_frames, max_tags, d_map, n_ids, d_rig, tag_size, max_iters, sigma_px, d_rig_out, d_result, d_cov, d_poses}, stream);
}

extern "C" int asl_calibrate_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                       const asl_rig_camera *rig, double tag_size, int max_iters, double sigma_px, asl_rig_camera *rig_out,
                                       asl_rig_calib_result *result, asl_pose_cov *cov, asl_cam_pose *poses)
{
    return rig_calibrate_batch(d, {obs, n_cams, n_frames, max_tags, map, n_ids, rig, tag_size, max_iters, sigma_px, rig_out, result, cov, poses});
}

// ---- mapping (k_map.inc)

// One map call, in the robust entry points' argument order; the plain ones give huber_px 0 and no slot_weight.  tag_std
// and slot_weight may be NULL: not asked for.  The single-camera forms leave n_cams 0 and rig NULL; the rig forms
// (asl_map_rig_*) give n_cams and the table and leave cam's K and dist NULL, n_dist 0; their block is camera-major and their
// slot weights n_cams x n_frames x max_tags.  obs, rig, map, tag_std, poses, result and slot_weight are all host (*_batch) or
// all device pointers (*_frames_device).  tag_sizes (the sized forms; NULL: no table) is a host array of n_ids in both,
// like K and dist: the side of each id, 0 for the call's tag_size.  The covariance forms (asl_mapcov_*, asl_mapcov_rig_*)
// set with_cov and give cov_slot (n_ids int32), map_cov (doubles, leading dimension 6 * cap_tags) and cap_tags, host or
// device as the rest; every other form leaves them NULL, 0 and false.
struct MapCall {
    const void *obs; int n_cams, n_frames, max_tags, n_ids;
    const void *rig; Camera cam; const float *tag_sizes;
    int world_id; double huber_px; int max_iters;
    void *map, *tag_std, *poses, *result, *slot_weight;
    void *cov_slot, *map_cov; int cap_tags;
    bool with_cov;      // a covariance form: cov_slot and map_cov must be there
};

static bool is_rig(const MapCall &c) { return c.n_cams || c.rig; }

// every refusal that needs no look at the block, before anything is written or enqueued; the same for both forms, but that
// a rig's table, checked last, is read back first where the pointers are the device's (check_localize_call's rule)
static int check_map_call(const asl_detector *d, const MapCall &c, bool device)
{
    const bool rig = is_rig(c);
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !(rig ? c.rig : (const void *)c.cam.K) || !c.map || !c.poses || !c.result) return fail(ASL_EINVAL, "NULL argument");
    if (c.with_cov && (!c.cov_slot || !c.map_cov)) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_frames < 1) return fail(ASL_EINVAL, "n_frames must be >= 1 (got %d)", c.n_frames);
    if (rig && (c.n_cams < 1 || c.n_cams > RIG_MAX_CAMS)) return fail(ASL_EINVAL, "n_cams must be in [1, %d] (got %d)", RIG_MAX_CAMS, c.n_cams);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, c.cam)) return rc;
    if (rig && c.n_cams * c.max_tags > RIG_MAX_SLOTS)
        return fail(ASL_EINVAL, "n_cams * max_tags must be <= %d (got %d x %d)", RIG_MAX_SLOTS, c.n_cams, c.max_tags);
    if (c.world_id < -1 || c.world_id >= c.n_ids) return fail(ASL_EINVAL, "world_id must be -1 or in [0, n_ids) (got %d)", c.world_id);
    if (c.max_iters < 1 || c.max_iters > MAP_MAX_ITERS) return fail(ASL_EINVAL, "max_iters must be in [1, %d] (got %d)", MAP_MAX_ITERS, c.max_iters);
    if (!(c.huber_px >= 0) || !std::isfinite(c.huber_px)) return fail(ASL_EINVAL, "huber_px must be >= 0 and finite (got %g)", c.huber_px);
    for (int i = 0; c.tag_sizes && i < c.n_ids; i++)
        if (!(c.tag_sizes[i] >= 0) || !std::isfinite(c.tag_sizes[i]))
            return fail(ASL_EINVAL, "tag_sizes[%d] must be 0 or positive and finite (got %g)", i, (double)c.tag_sizes[i]);
    if (c.with_cov && c.cap_tags < 1) return fail(ASL_EINVAL, "cap_tags must be >= 1 (got %d)", c.cap_tags);
    if (!rig) return ASL_OK;
    asl_rig_camera tab[RIG_MAX_CAMS];
    if (device) {
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipMemcpy(tab, c.rig, sizeof(asl_rig_camera) * (size_t)c.n_cams, hipMemcpyDeviceToHost));
    }
    return check_rig_table(device ? tab : (const asl_rig_camera *)c.rig, c.n_cams);
}

// c's pointers are the device's; RIG: the kernels' view model (k_map.inc)
template <bool RIG>
static int launch_map_views(asl_detector *d, const MapCall &c, hipStream_t st)
{
    const size_t nf = (size_t)c.n_frames, ni = (size_t)c.n_ids, nsl = (RIG ? (size_t)c.n_cams : 1) * nf * (size_t)c.max_tags;
    MapArgs a{};
    int *per_id, *per_frame, *per_cam, *per_obs, *csr;  // the grouped int arrays, one piece per group
    double *cams, *cov_s2;
    float *sizes;
    int *cov_tag;  // the covariance calls': the tag of each block, then the number of blocks
    if (carve_ws(d->map_ws, [&](WsCarve &w) {
            a.head = w.take<MapHead>(1); per_id = w.take<int>(5 * (ni + 1)); per_frame = w.take<int>(4 * (nf + 1));
            per_cam = w.take<int>(4 * (nf + 1)); a.tag_state = w.take<int>(ni + 1); a.slot_obs = w.take<int>(nsl); per_obs = w.take<int>(5 * nsl);
            csr = w.take<int>(3 * nsl + nf + 2 * ni + 3); a.W = w.take<double>(12 * nf); a.G = w.take<double>(12 * ni);
            cams = w.take<double>(RIG_CAM_DOUBLES * RIG_MAX_CAMS); a.tag_half = w.take<double>(ni); sizes = w.take<float>(ni);
            cov_s2 = w.take<double>(1); cov_tag = w.take<int>(ni + 1);
        }))
        return fail(ASL_ENOMEM, "map workspace allocation failed");
    a.obs = (const ObsRec *)c.obs; a.n_frames = c.n_frames; a.max_tags = c.max_tags; a.n_ids = c.n_ids; a.world_req = c.world_id;
    a.n_rig = RIG ? c.n_cams : 1; a.cams = RIG ? cams : nullptr; a.sizes = sizes;
    a.seen = per_id; a.id_tag = per_id + (ni + 1); a.tag_id = per_id + 2 * (ni + 1); a.tmp = per_id + 3 * (ni + 1); a.tmp2 = per_id + 4 * (ni + 1);
    a.fr_npart = per_frame; a.fr_cam = per_frame + (nf + 1); a.fr_obs0 = per_frame + 2 * (nf + 1); a.fr_ndist = per_frame + 3 * (nf + 1);
    a.cam_frame = per_cam; a.cam_ptr0 = per_cam + (nf + 1); a.cam_state = per_cam + 2 * (nf + 1); a.cam_seed = per_cam + 3 * (nf + 1);
    a.obs_slot = per_obs; a.obs_cam = per_obs + nsl; a.obs_tag = per_obs + 2 * nsl; a.obs_act = per_obs + 3 * nsl; a.obs_next = per_obs + 4 * nsl;
    a.cam_obs = csr; a.tag_obs = csr + nsl; a.ptag_obs = csr + 2 * nsl; a.cam_ptr = csr + 3 * nsl; a.tag_ptr = a.cam_ptr + nf + 1;
    a.ptag_ptr = a.tag_ptr + ni + 1;
    static const double no_K[9] = {};
    const CamDev cam = make_cam(d, RIG ? no_K : c.cam.K, c.cam.dist, c.cam.n_dist, c.cam.tag_size);   // a rig: for its half alone
    if (RIG) hipLaunchKernelGGL(k_map_rig_table, dim3(1), dim3(ASL_WAVE), 0, st, cams, (const RigCamRec *)c.rig, c.n_cams);

    // the per-id sizes: the caller's table or, without one, zeros (read before the wait below returns)
    if (c.tag_sizes) HIPCHK(hipMemcpyAsync(sizes, c.tag_sizes, sizeof(float) * ni, hipMemcpyHostToDevice, st));
    else HIPCHK(hipMemsetAsync(sizes, 0, sizeof(float) * ni, st));
    hipLaunchKernelGGL(k_map_gather, dim3(1), dim3(MAP_WG), 0, st, a, cam.half);
    MapHead h;
    HIPCHK(hipMemcpyAsync(&h, a.head, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the one wait before the end: the reduced system is sized by the tags seen
    const int NC = h.n_cams, NT = h.n_tags, NM = h.n_obs, WT = h.world_tag;
    auto finish_nothing = [&]() {
        hipLaunchKernelGGL(k_map_finish, dim3(1), dim3(MAP_WG), 0, st, a, NC, NT, NM, WT, 1, (const double *)nullptr, (const double *)nullptr,
                           (const double *)nullptr, (const double *)nullptr, (const int *)nullptr, (const double *)nullptr, (const double *)nullptr,
                           (MapTagRec *)c.map, (double *)c.tag_std, (CamPoseRec *)c.poses, (MapResultRec *)c.result, (double *)c.slot_weight,
                           (int *)c.cov_slot, cov_tag, cov_tag + ni, cov_s2);
        HIPCHK(hipGetLastError());
        return ASL_OK;
    };
    if (NT > MAP_MAX_TAGS) return fail(ASL_EINVAL, "the frames see %d tags; the map's dense reduced system takes at most %d", NT, MAP_MAX_TAGS);
    if (c.with_cov && NT - 1 > c.cap_tags)
        return fail(ASL_EINVAL, "the frames see %d tags besides the world tag; the covariance matrix holds cap_tags = %d", NT - 1, c.cap_tags);
    if (WT < 0) {
        int rc = finish_nothing();
        if (rc) return rc;
        if (c.world_id >= 0) return fail(ASL_EINVAL, "world tag %d is not seen by any frame with 2 or more taking-part slots", c.world_id);
        return ASL_OK;
    }

    // the problem-sized part: the LM's buffers (gn_lm_carve), the seed costs, the std, the robust call's weights and sums;
    // the reduced system reads the LM's copies of the list offsets (k_map_park empties them after the stop)
    const int n = 6 * NT;
    const size_t nc = (size_t)NC, nt = (size_t)NT, nm = (size_t)NM;
    GnSystem sys = {nullptr, nullptr, a.cam_obs, nullptr, a.ptag_obs, a.obs_cam, a.obs_tag, nullptr, NC, NT, WT};  // the pair lists
    GnLmBufs b;
    const bool robust = c.huber_px > 0;  // 0: the plain kernels
    double *seed_obs, *var, *wmin_obs = nullptr, *soft = nullptr, *Yt = nullptr;
    if (carve_ws(d->map_lm, [&](WsCarve &w) {
            b = gn_lm_carve(w, sys, NM, 2 * MAP_LM__N);
            seed_obs = w.take<double>(nm); var = w.take<double>(n); sys.cam_ptr = w.take<int>(nc + 1); sys.tag_ptr = w.take<int>(nt + 1);
            if (robust) { wmin_obs = w.take<double>(nm); soft = w.take<double>(MAP_SOFT__N); }
            if (c.with_cov) Yt = w.take<double>((size_t)n * n);  // the columns of L^-1, one per row
        }))
        return fail(ASL_ENOMEM, "map workspace allocation failed");
    a.obs_of = sys.obs_of;
    double *lm = b.lm, *lm0 = lm + MAP_LM__N;
    const dim3 wg(MAP_WG);

    range_push("map: seed");
    hipLaunchKernelGGL(k_map_csr, dim3(1), wg, 0, st, a, NC, NT);
    hipLaunchKernelGGL(k_map_chain<RIG>, dim3(1), wg, 0, st, a, NC, NT, NM, WT, cam.half);
    hipLaunchKernelGGL(k_map_csr, dim3(1), wg, 0, st, a, NC, NT);
    for (int sw = 0; sw < 2; sw++) {
        hipLaunchKernelGGL(k_map_sweep_cam<RIG>, dim3(NC), dim3(ASL_WAVE), loc_lds_bytes(a.n_rig * c.max_tags), st, a, cam);
        hipLaunchKernelGGL(k_map_sweep_tag<RIG>, dim3(NT), dim3(ASL_WAVE), 0, st, a, cam);
    }
    hipLaunchKernelGGL(k_map_gauge, dim3(1), wg, 0, st, a, NC, NT, WT);
    hipLaunchKernelGGL(k_map_flip<RIG>, dim3(NT), dim3(ASL_WAVE), 0, st, a, cam, WT);
    hipLaunchKernelGGL(k_map_behind<RIG>, dim3((NC + 63) / 64), dim3(64), 0, st, a, NC);
    hipLaunchKernelGGL(k_map_csr, dim3(1), wg, 0, st, a, NC, NT);
    hipLaunchKernelGGL(k_map_lm_init, dim3(1), dim3(1), 0, st, (const MapHead *)a.head, lm, lm0);
    HIPCHK(hipMemsetAsync(b.flag, 0, 8, st));
    range_pop();

    range_push("map: LM");
    auto lin = [&](const double *W, const double *G, double *D, int force) {
        const auto kernel = robust ? k_map_linearize<true, RIG> : k_map_linearize<false, RIG>;
        hipLaunchKernelGGL(kernel, dim3((NM + 3) / 4), dim3(256), 0, st, a, W, G, NM, cam, D, b.cost_obs, lm, force, c.huber_px);
        if (RIG) hipLaunchKernelGGL(k_map_fold, dim3(NM), dim3(256), 0, st, a, NM, NT, D, (const double *)lm, force);
    };
    auto decide = [&]() { hipLaunchKernelGGL(k_map_decide, dim3(1), dim3(1), 0, st, lm, b.flag); };
    auto park = [&]() {
        hipLaunchKernelGGL(k_map_park, dim3((NC + NT + 2 + 255) / 256), dim3(256), 0, st, lm, sys.cam_ptr, NC, sys.tag_ptr, NT);
    };
    HIPCHK(hipMemcpyAsync(sys.cam_ptr, a.cam_ptr, 4 * (nc + 1), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(sys.tag_ptr, a.ptag_ptr, 4 * (nt + 1), hipMemcpyDeviceToDevice, st));
    int rc = gn_lm_run(sys, b, a.W, a.G, NM, c.max_iters, seed_obs, lin, decide, park, st);
    if (rc) return rc;
    // the final state's per-observation costs (and its blocks again, for the std)
    lin(a.W, a.G, sys.D, 1);
    if (robust) hipLaunchKernelGGL(k_map_soft<RIG>, dim3(1), dim3(256), 0, st, a, NM, cam, c.huber_px, wmin_obs, soft);
    range_pop();
    const bool want_var = c.tag_std || c.with_cov;
    if (want_var) {
        GnSystem full = sys;  // undamped, over every active observation
        full.cam_ptr = a.cam_ptr;
        full.tag_ptr = a.ptag_ptr;
        rc = gn_factor_step(full, lm0, b.flag + 1, st);
        if (rc) return rc;
        if (c.with_cov) hipLaunchKernelGGL(k_map_cols, dim3(n), dim3(256), (size_t)n * sizeof(double), st, sys.S, sys.Linv, n, var, Yt);
        else hipLaunchKernelGGL(k_map_std, dim3(n), dim3(256), (size_t)n * sizeof(double), st, sys.S, sys.Linv, n, var);
    }
    hipLaunchKernelGGL(k_map_finish, dim3(1), wg, 0, st, a, NC, NT, NM, WT, 0, lm, b.cost_obs, seed_obs, want_var ? var : nullptr, b.flag + 1,
                       (const double *)wmin_obs, (const double *)soft, (MapTagRec *)c.map, (double *)c.tag_std, (CamPoseRec *)c.poses,
                       (MapResultRec *)c.result, (double *)c.slot_weight, (int *)c.cov_slot, cov_tag, cov_tag + ni, cov_s2);
    if (c.with_cov && NT > 1) {  // the blocks k_map_finish numbered: at most NT - 1 of them
        const unsigned int tiles = (unsigned int)((6 * (NT - 1) + MAP_COV_T - 1) / MAP_COV_T);
        hipLaunchKernelGGL(k_map_cov_gram, dim3(tiles, tiles), dim3(256), 0, st, (const double *)Yt, n, (const int *)cov_tag,
                           (const int *)(cov_tag + ni), (const double *)cov_s2, (double *)c.map_cov, 6 * c.cap_tags);
    }
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static int launch_map(asl_detector *d, const MapCall &c, hipStream_t st)
{
    return is_rig(c) ? launch_map_views<true>(d, c, st) : launch_map_views<false>(d, c, st);
}

static constexpr auto map_frames_device = frames_device<MapCall, check_map_call, launch_map>;

// the host forms; a rig's table is staged in solve_out too
static int map_batch(asl_detector *d, const MapCall &c)
{
    if (int rc = check_map_call(d, c, false)) return rc;
    const bool rig = is_rig(c);
    const size_t ni = (size_t)c.n_ids, rows = (size_t)(rig ? c.n_cams : 1) * (size_t)c.n_frames, rig_bytes = sizeof(asl_rig_camera) * (size_t)c.n_cams;
    OutPiece o[] = {{c.result, sizeof(asl_map_result)}, {c.map, sizeof(asl_map_tag) * ni}, {c.tag_std, c.tag_std ? sizeof(double) * 6 * ni : 0},
                    {c.poses, sizeof(asl_cam_pose) * (size_t)c.n_frames},
                    {c.slot_weight, c.slot_weight ? sizeof(double) * rows * (size_t)c.max_tags : 0}, {nullptr, rig_bytes},
                    {c.cov_slot, c.with_cov ? sizeof(int32_t) * ni : 0}, {nullptr, 0}};
    // the covariance is staged at the most blocks the call can have (cap_tags, and no more than the ids or the solver's
    // tags), with that as its leading dimension; only the region written goes back, into the caller's leading dimension
    const int cap = c.with_cov ? (int)std::min<size_t>({(size_t)c.cap_tags, ni, (size_t)MAP_MAX_TAGS}) : 0;
    o[7].bytes = sizeof(double) * 36 * (size_t)cap * (size_t)cap;
    if (int rc = stage_host_call(d, rig ? "rig map" : "map", o, c.obs, (int)rows, c.max_tags, nullptr, c.n_ids)) return rc;
    if (rig) HIPCHK(hipMemcpy(o[5].dev, c.rig, rig_bytes, hipMemcpyHostToDevice));
    MapCall dc = c;
    dc.obs = d->loc_obs.p; dc.result = o[0].dev; dc.map = o[1].dev; dc.tag_std = o[2].dev; dc.poses = o[3].dev; dc.slot_weight = o[4].dev;
    dc.rig = o[5].dev; dc.cov_slot = o[6].dev; dc.map_cov = o[7].dev; dc.cap_tags = cap;
    if (int rc = launch_map(d, dc, nullptr)) return rc;
    if (int rc = fetch_out(o)) return rc;
    if (c.with_cov) {
        const int32_t *slot = (const int32_t *)c.cov_slot;
        size_t n_cov = 0;
        for (size_t i = 0; i < ni; i++) n_cov += slot[i] >= 0;
        if (n_cov)
            HIPCHK(hipMemcpy2D(c.map_cov, sizeof(double) * 6 * (size_t)c.cap_tags, o[7].dev, sizeof(double) * 6 * (size_t)cap, sizeof(double) * 6 * n_cov,
                               6 * n_cov, hipMemcpyDeviceToHost));
    }
    return ASL_OK;
}

extern "C" int asl_map_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K, const double *dist,
                                     int n_dist, double tag_size, int world_id, int max_iters, void *d_map, void *d_tag_std, void *d_poses,
                                     void *d_result, void *stream)
{
    return map_frames_device(d, {d_obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, nullptr, world_id, 0.0, max_iters, d_map, d_tag_std, d_poses, d_result, nullptr}, stream);
}

extern "C" int asl_map_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K, const double *dist,
                             int n_dist, double tag_size, int world_id, int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses,
                             asl_map_result *result)
{
    return map_batch(d, {obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, nullptr, world_id, 0.0, max_iters, map, tag_std, poses, result, nullptr});
}

extern "C" int asl_map_robust_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                                            const double *dist, int n_dist, double tag_size, int world_id, double huber_px, int max_iters,
                                            void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight, void *stream)
{
    return map_frames_device(d, {d_obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, nullptr, world_id, huber_px, max_iters, d_map, d_tag_std, d_poses,
                                 d_result, d_slot_weight}, stream);
}

extern "C" int asl_map_robust_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K, const double *dist,
                                    int n_dist, double tag_size, int world_id, double huber_px, int max_iters, asl_map_tag *map, double *tag_std,
                                    asl_cam_pose *poses, asl_map_result *result, double *slot_weight)
{
    return map_batch(d, {obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, nullptr, world_id, huber_px, max_iters, map, tag_std, poses, result,
                         slot_weight});
}

extern "C" int asl_map_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids, const void *d_rig,
                                         double tag_size, int world_id, double rig_huber_px, int max_iters, void *d_map, void *d_tag_std,
                                         void *d_poses, void *d_result, void *d_slot_weight, void *stream)
{
    return map_frames_device(d, {d_obs, n_cams, n_frames, max_tags, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, nullptr, world_id, rig_huber_px, max_iters,
                                 d_map, d_tag_std, d_poses, d_result, d_slot_weight}, stream);
}

extern "C" int asl_map_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids, const asl_rig_camera *rig,
                                 double tag_size, int world_id, double rig_huber_px, int max_iters, asl_map_tag *map, double *tag_std,
                                 asl_cam_pose *poses, asl_map_result *result, double *slot_weight)
{
    return map_batch(d, {obs, n_cams, n_frames, max_tags, n_ids, rig, {nullptr, nullptr, 0, tag_size}, nullptr, world_id, rig_huber_px, max_iters, map, tag_std,
                         poses, result, slot_weight});
}

// The sized forms: the robust and the rig argument lists with the per-id size table after tag_size.
extern "C" int asl_map_sized_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                                           const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id,
                                           double sized_huber_px, int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result,
                                           void *d_slot_weight, void *stream)
{
    return map_frames_device(d, {d_obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, tag_sizes, world_id, sized_huber_px, max_iters,
                                 d_map, d_tag_std, d_poses, d_result, d_slot_weight}, stream);
}

extern "C" int asl_map_sized_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K, const double *dist,
                                   int n_dist, double tag_size, const float *tag_sizes, int world_id, double sized_huber_px, int max_iters,
                                   asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result, double *slot_weight)
{
    return map_batch(d, {obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, tag_sizes, world_id, sized_huber_px, max_iters, map,
                         tag_std, poses, result, slot_weight});
}

extern "C" int asl_map_rig_sized_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                               const void *d_rig, double tag_size, const float *tag_sizes, int world_id, double sized_huber_px,
                                               int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight,
                                               void *stream)
{
    return map_frames_device(d, {d_obs, n_cams, n_frames, max_tags, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, tag_sizes, world_id, sized_huber_px,
                                 max_iters, d_map, d_tag_std, d_poses, d_result, d_slot_weight}, stream);
}

extern "C" int asl_map_rig_sized_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                       const asl_rig_camera *rig, double tag_size, const float *tag_sizes, int world_id, double sized_huber_px,
                                       int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result,
                                       double *slot_weight)
{
    return map_batch(d, {obs, n_cams, n_frames, max_tags, n_ids, rig, {nullptr, nullptr, 0, tag_size}, tag_sizes, world_id, sized_huber_px, max_iters, map,
                         tag_std, poses, result, slot_weight});
}

// The covariance forms: the sized argument lists with the joint covariance of the map after slot_weight.
extern "C" int asl_mapcov_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                                         const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id,
                                         double cov_huber_px, int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result,
                                         void *d_slot_weight, void *d_cov_slot, void *d_map_cov, int cap_tags, void *stream)
{
    return map_frames_device(d, {d_obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, tag_sizes, world_id, cov_huber_px, max_iters,
                                 d_map, d_tag_std, d_poses, d_result, d_slot_weight, d_cov_slot, d_map_cov, cap_tags, true}, stream);
}

extern "C" int asl_mapcov_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K, const double *dist,
                                 int n_dist, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px, int max_iters,
                                 asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result, double *slot_weight,
                                 int32_t *cov_slot, double *map_cov, int cap_tags)
{
    return map_batch(d, {obs, 0, n_frames, max_tags, n_ids, nullptr, {K, dist, n_dist, tag_size}, tag_sizes, world_id, cov_huber_px, max_iters, map,
                         tag_std, poses, result, slot_weight, cov_slot, map_cov, cap_tags, true});
}

extern "C" int asl_mapcov_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                             const void *d_rig, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px,
                                             int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight,
                                             void *d_cov_slot, void *d_map_cov, int cap_tags, void *stream)
{
    return map_frames_device(d, {d_obs, n_cams, n_frames, max_tags, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, tag_sizes, world_id, cov_huber_px,
                                 max_iters, d_map, d_tag_std, d_poses, d_result, d_slot_weight, d_cov_slot, d_map_cov, cap_tags, true}, stream);
}

extern "C" int asl_mapcov_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                     const asl_rig_camera *rig, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px,
                                     int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result,
                                     double *slot_weight, int32_t *cov_slot, double *map_cov, int cap_tags)
{
    return map_batch(d, {obs, n_cams, n_frames, max_tags, n_ids, rig, {nullptr, nullptr, 0, tag_size}, tag_sizes, world_id, cov_huber_px, max_iters, map,
                         tag_std, poses, result, slot_weight, cov_slot, map_cov, cap_tags, true});
}

// ---- sequence localisation with a motion prior (k_smooth.inc)

#define SMOOTH_SEQ_FRAMES 65535   // frames of one sequence
#define SMOOTH_SEQS 65535         // sequences of one call
#define SMOOTH_FRAMES 1048576     // frames of one call: the work buffers, about 3.6 KB a frame, stay under 4 GB

// One smoothing call, whichever of the twelve entry points made it, in their argument order (n_cams and rig, which only the
// rig pair gives, stand last: the ten single-camera forms leave them 0 and NULL).  The single-sequence forms leave
// seq_start NULL, n_seq 1 and sequences false: the one sequence {0, n_frames}; seq_start is a host array of n_seq + 1
// offsets in every form.  The plain forms leave cov NULL and with_cov false; the sequences forms set with_cov where cov is
// given.  The host forms may leave seed NULL: the per-frame localisation of the same block.  obs, map, seed, out, result
// and cov are all host or all device pointers.  huber_px: 0 from the six plain entry points (the squared corner loss and
// its kernels), the robust and the timed pairs' threshold in pixels otherwise.  times: NULL from the eight entry points
// without it (frame f is at time f), the timed pair's n_frames doubles otherwise, a host or a device array as the rest.
// The rig pair (asl_smooth_rig_sequences_*) gives n_cams and the camera table, host or device as the rest, as LocCall
// carries them, and leaves cam's K and dist NULL, n_dist 0; obs is then the camera-major block of n_cams * n_frames rows.
struct SmoothCall {
    const void *obs; int n_frames, max_tags;
    const void *map; int n_ids;
    Camera cam;
    const void *seed, *times; const int32_t *seq_start; int n_seq;
    double sigma_px, sigma_rot, sigma_trans, huber_px; int max_iters;
    void *out, *result, *cov;
    bool with_cov, sequences;
    int n_cams; const void *rig;
};

static bool is_rig(const SmoothCall &c) { return c.n_cams || c.rig; }

static bool smooth_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every refusal, before anything is written or enqueued.  device: the seed must be there, and the outputs apart from it,
// from the times and from each other (host arrays are apart by contract).  The times' values are the device's to judge.
// A rig's table is checked last, as check_localize_call checks it: where it is, or (device) in a copy read back.
static int check_smooth_call(const asl_detector *d, const SmoothCall &c, bool device)
{
    const bool rig = is_rig(c);
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.map || !(rig ? c.rig : (const void *)c.cam.K) || !c.out || !c.result || (c.sequences && !c.seq_start))
        return fail(ASL_EINVAL, "NULL argument");
    const int most = c.sequences ? SMOOTH_FRAMES : SMOOTH_SEQ_FRAMES;
    if (c.n_frames < 1 || c.n_frames > most) return fail(ASL_EINVAL, "n_frames must be in [1, %d] (got %d)", most, c.n_frames);
    if (c.sequences) {
        if (c.n_seq < 1 || c.n_seq > SMOOTH_SEQS) return fail(ASL_EINVAL, "n_seq must be in [1, %d] (got %d)", SMOOTH_SEQS, c.n_seq);
        if (c.seq_start[0] != 0 || c.seq_start[c.n_seq] != c.n_frames)
            return fail(ASL_EINVAL, "seq_start must run from 0 to n_frames (got %d to %d, n_frames %d)", c.seq_start[0], c.seq_start[c.n_seq], c.n_frames);
        for (int k = 0; k < c.n_seq; k++) {
            const int64_t len = (int64_t)c.seq_start[k + 1] - c.seq_start[k];
            if (len < 1 || len > SMOOTH_SEQ_FRAMES) return fail(ASL_EINVAL, "sequence %d must have 1 to %d frames (got %lld)", k, SMOOTH_SEQ_FRAMES, (long long)len);
        }
    }
    if (rig && (c.n_cams < 1 || c.n_cams > RIG_MAX_CAMS)) return fail(ASL_EINVAL, "n_cams must be in [1, %d] (got %d)", RIG_MAX_CAMS, c.n_cams);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, c.cam)) return rc;
    if (rig && c.n_cams * c.max_tags > RIG_MAX_SLOTS)
        return fail(ASL_EINVAL, "n_cams * max_tags must be <= %d (got %d x %d)", RIG_MAX_SLOTS, c.n_cams, c.max_tags);
    for (int k = 0; !rig && k < 9; k++)
        if (!std::isfinite(c.cam.K[k])) return fail(ASL_EINVAL, "K is not finite");
    for (double s : {c.sigma_px, c.sigma_rot, c.sigma_trans})
        if (!(s > 0) || !std::isfinite(s)) return fail(ASL_EINVAL, "sigma_px, sigma_rot and sigma_trans must be positive and finite (got %g)", s);
    if (!(c.huber_px >= 0) || !std::isfinite(c.huber_px)) return fail(ASL_EINVAL, "huber_px must be finite and not negative (got %g)", c.huber_px);
    if (c.max_iters < 1 || c.max_iters > 100) return fail(ASL_EINVAL, "max_iters must be in [1, 100] (got %d)", c.max_iters);
    if ((device && !c.seed) || (c.with_cov && !c.cov)) return fail(ASL_EINVAL, "NULL argument");
    if (!device) return rig ? check_rig_table((const asl_rig_camera *)c.rig, c.n_cams) : ASL_OK;
    const size_t poses = sizeof(asl_cam_pose) * (size_t)c.n_frames, covs = sizeof(asl_pose_cov) * (size_t)c.n_frames;
    if (smooth_overlap(c.seed, poses, c.out, poses)) return fail(ASL_EINVAL, "d_out overlaps d_seed");
    if (c.with_cov && (smooth_overlap(c.cov, covs, c.out, poses) || smooth_overlap(c.cov, covs, c.seed, poses)))
        return fail(ASL_EINVAL, "d_cov overlaps d_out or d_seed");
    const size_t times = sizeof(double) * (size_t)c.n_frames;
    if (c.times && (smooth_overlap(c.times, times, c.out, poses) || (c.with_cov && smooth_overlap(c.times, times, c.cov, covs))))
        return fail(ASL_EINVAL, "d_times overlaps d_out or d_cov");
    if (!rig) return ASL_OK;
    asl_rig_camera tab[RIG_MAX_CAMS];
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemcpy(tab, c.rig, sizeof(asl_rig_camera) * (size_t)c.n_cams, hipMemcpyDeviceToHost));
    return check_rig_table(tab, c.n_cams);
}

// c's pointers are the device's but seq_start (host, not read for n_seq 1); everything is enqueued on st, nothing waits.
// cov: NULL, or the frames' asl_pose_cov (two more launches).  n_seq > 1: k_smooth_seqs first, a launch per SM_SEQ_CHUNK
// sequences, which carries the offsets to the device in its arguments.  huber_px > 0: the robust instantiations of the two
// kernels that cost corners, the same launches otherwise.  times: carried in SmoothBufs, the same launches.  A rig: those two
// kernels are k_smooth_rig_cand and k_smooth_rig_lin over the camera-major block, with the rig's LDS; nothing else differs.
static int launch_smooth(asl_detector *d, const SmoothCall &c, hipStream_t st)
{
    const size_t n = (size_t)c.n_frames, ns = (size_t)c.n_seq;
    SmoothBufs b{};
    b.n = c.n_frames; b.n_seq = c.n_seq; b.times = (const double *)c.times;
    if (carve_ws(d->smooth_ws, [&](WsCarve &ws) {
            b.cand = ws.take<double>(24 * n); b.dcost = ws.take<double>(2 * n); b.tcost = ws.take<double>(4 * n);
            b.posed = ws.take<int>(n); b.ntags = ws.take<int>(n); b.src = ws.take<int>(n); b.back = ws.take<int>(n); b.choice = ws.take<int>(n);
            b.code = ws.take<int>(n); b.head = ws.take<int>(SMH__N * ns); b.lm = ws.take<double>(SM__N * ns); b.cseed = ws.take<double>(n);
            b.delta = ws.take<double>(6 * n); b.fac = ws.take<double>(SM_FAC * n);
            b.set[0] = ws.take<double>(SM_SET * n); b.set[1] = ws.take<double>(SM_SET * n);
            if (c.n_seq > 1) { b.seq = ws.take<int>(ns + 1); b.fseq = ws.take<int>(n); }
        }))
        return fail(ASL_ENOMEM, "sequence localisation workspace allocation failed");
    static const double no_K[9] = {};
    const bool rig = is_rig(c);
    const CamDev cam = make_cam(d, rig ? no_K : c.cam.K, c.cam.dist, c.cam.n_dist, c.cam.tag_size);   // a rig: for its half alone
    const ObsRec *obs = (const ObsRec *)c.obs;
    const MapTagRec *map = (const MapTagRec *)c.map;
    const RigCamRec *tab = (const RigCamRec *)c.rig;
    const CamPoseRec *seed = (const CamPoseRec *)c.seed;
    const double w = 1.0 / (c.sigma_px * c.sigma_px), isr = 1.0 / c.sigma_rot, ist = 1.0 / c.sigma_trans;
    const size_t lds = rig ? rig_lds_bytes(c.n_cams, c.max_tags) : loc_lds_bytes(c.max_tags);
    const dim3 frames((unsigned int)c.n_frames), wave(ASL_WAVE), seqs((unsigned int)c.n_seq), wg(SM_WG), per_thread((unsigned int)((n + SM_WG - 1) / SM_WG));

    static_assert(SM_SET <= SM_WG, "k_smooth_commit: a thread an entry of a frame");
    const dim3 commit_blocks((unsigned int)std::min<size_t>(n, 1024));

    range_push("smooth: seed chain");
    for (int k0 = 0; c.n_seq > 1 && k0 < c.n_seq; k0 += SM_SEQ_CHUNK) {
        SmoothSeqChunk ch;
        ch.k0 = k0;
        ch.count = std::min(c.n_seq - k0, SM_SEQ_CHUNK);
        memcpy(ch.start, c.seq_start + k0, sizeof(int32_t) * ((size_t)ch.count + 1));
        hipLaunchKernelGGL(k_smooth_seqs, dim3((unsigned int)ch.count), wg, 0, st, b, ch);
    }
    const bool robust = c.huber_px > 0;
    const auto cand = robust ? k_smooth_cand<true> : k_smooth_cand<false>;
    const auto lin = robust ? k_smooth_lin<true> : k_smooth_lin<false>;
    const auto rig_cand = robust ? k_smooth_rig_cand<true> : k_smooth_rig_cand<false>;
    const auto rig_lin = robust ? k_smooth_rig_lin<true> : k_smooth_rig_lin<false>;
    const auto linearise = [&](int trial) {
        if (rig)
            hipLaunchKernelGGL(rig_lin, frames, wave, lds, st, obs, c.n_cams, c.n_frames, c.max_tags, map, c.n_ids, tab, cam.half, b, trial, isr, ist,
                               c.huber_px);
        else
            hipLaunchKernelGGL(lin, frames, wave, lds, st, obs, c.max_tags, map, c.n_ids, cam, b, trial, isr, ist, c.huber_px);
    };
    if (rig)
        hipLaunchKernelGGL(rig_cand, frames, wave, lds, st, obs, c.n_cams, c.n_frames, c.max_tags, map, c.n_ids, tab, cam.half, seed, w, b, c.huber_px);
    else
        hipLaunchKernelGGL(cand, frames, wave, lds, st, obs, c.max_tags, map, c.n_ids, cam, seed, w, b, c.huber_px);
    hipLaunchKernelGGL(k_smooth_scan, seqs, wave, 0, st, b);
    hipLaunchKernelGGL(k_smooth_trans, dim3((unsigned int)((n + ASL_WAVE - 1) / ASL_WAVE)), wave, 0, st, b, isr, ist);
    hipLaunchKernelGGL(k_smooth_dp, seqs, wave, 0, st, b);
    hipLaunchKernelGGL(k_smooth_fill, per_thread, wg, 0, st, b, seed);
    linearise(0);
    hipLaunchKernelGGL(k_smooth_init, seqs, wg, 0, st, b, w);
    range_pop();
    range_push("smooth: LM");
    for (int it = 0; it < c.max_iters; it++) {
        hipLaunchKernelGGL(k_smooth_solve, seqs, wave, 0, st, b, w);
        linearise(1);
        hipLaunchKernelGGL(k_smooth_decide, seqs, wg, 0, st, b, w);
        hipLaunchKernelGGL(k_smooth_commit, commit_blocks, wg, 0, st, b);
    }
    hipLaunchKernelGGL(k_smooth_finish, per_thread, wg, 0, st, b, (CamPoseRec *)c.out, (SmoothResultRec *)c.result);
    range_pop();
    if (c.cov) {
        range_push("smooth: covariance");
        hipLaunchKernelGGL(k_smooth_cov, seqs, wave, 0, st, b, w, (PoseCovRec *)c.cov);
        hipLaunchKernelGGL(k_smooth_cov_finish, per_thread, wg, 0, st, b, c.sigma_px, (PoseCovRec *)c.cov);
        range_pop();
    }
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

static constexpr auto smooth_frames_device = frames_device<SmoothCall, check_smooth_call, launch_smooth>;   // the six device forms

// the six host forms; a seed not given is the per-frame localisation of the same block (a rig: the rig localisation), gate 0;
// times and a rig's table are staged as a seed is
static int smooth_batch(asl_detector *d, const SmoothCall &c)
{
    if (int rc = check_smooth_call(d, c, false)) return rc;
    const size_t poses = sizeof(asl_cam_pose) * (size_t)c.n_frames;
    OutPiece o[] = {{c.result, sizeof(asl_smooth_result) * (size_t)c.n_seq}, {c.out, poses}, {nullptr, poses},
                    {c.cov, c.cov ? sizeof(asl_pose_cov) * (size_t)c.n_frames : 0}, {nullptr, c.times ? sizeof(double) * (size_t)c.n_frames : 0},
                    {nullptr, sizeof(asl_rig_camera) * (size_t)c.n_cams}};
    const bool rig = is_rig(c);
    if (int rc = stage_host_call(d, "sequence localisation", o, c.obs, (rig ? c.n_cams : 1) * c.n_frames, c.max_tags, c.map, c.n_ids)) return rc;
    SmoothCall dc = c;
    dc.obs = d->loc_obs.p; dc.map = d->loc_map.p; dc.result = o[0].dev; dc.out = o[1].dev; dc.seed = o[2].dev; dc.cov = o[3].dev; dc.times = o[4].dev;
    dc.rig = o[5].dev;
    if (c.times) HIPCHK(hipMemcpy(o[4].dev, c.times, o[4].bytes, hipMemcpyHostToDevice));
    if (rig) HIPCHK(hipMemcpy(o[5].dev, c.rig, o[5].bytes, hipMemcpyHostToDevice));
    if (c.seed)
        HIPCHK(hipMemcpy(o[2].dev, c.seed, poses, hipMemcpyHostToDevice));
    else if (int rc = launch_localize(d, {dc.obs, c.n_cams, c.n_frames, c.max_tags, dc.map, c.n_ids, dc.rig, c.cam, 0.0, 0.0, o[2].dev, nullptr, false}, nullptr))
        return rc;
    if (int rc = launch_smooth(d, dc, nullptr)) return rc;
    return fetch_out(o);
}

extern "C" int asl_smooth_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                        const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed, double sigma_px,
                                        double sigma_rot, double sigma_trans, int max_iters, void *d_out, void *d_result, void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {K, dist, n_dist, tag_size}, d_seed, nullptr, nullptr, 1,
                                    sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, d_out, d_result, nullptr, false, false}, stream);
}

extern "C" int asl_smooth_cov_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                            const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                            double sigma_px, double sigma_rot, double sigma_trans, int max_iters, void *d_out, void *d_result,
                                            void *d_cov, void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {K, dist, n_dist, tag_size}, d_seed, nullptr, nullptr, 1,
                                    sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, d_out, d_result, d_cov, true, false}, stream);
}

extern "C" int asl_smooth_sequences_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                           const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                           const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                           int max_iters, void *d_out, void *d_results, void *d_cov, void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {K, dist, n_dist, tag_size}, d_seed, nullptr, seq_start, n_seq,
                                    sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, d_out, d_results, d_cov, d_cov != nullptr, true}, stream);
}

extern "C" int asl_smooth_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed, double sigma_px,
                                double sigma_rot, double sigma_trans, int max_iters, asl_cam_pose *out, asl_smooth_result *result)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {K, dist, n_dist, tag_size}, seed, nullptr, nullptr, 1,
                            sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, out, result, nullptr, false, false});
}

extern "C" int asl_smooth_cov_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                    const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed, double sigma_px,
                                    double sigma_rot, double sigma_trans, int max_iters, asl_cam_pose *out, asl_smooth_result *result,
                                    asl_pose_cov *cov)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {K, dist, n_dist, tag_size}, seed, nullptr, nullptr, 1,
                            sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, out, result, cov, true, false});
}

extern "C" int asl_smooth_sequences_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                          const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                                          const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                          int max_iters, asl_cam_pose *out, asl_smooth_result *results, asl_pose_cov *cov)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {K, dist, n_dist, tag_size}, seed, nullptr, seq_start, n_seq,
                            sigma_px, sigma_rot, sigma_trans, 0.0, max_iters, out, results, cov, cov != nullptr, true});
}

extern "C" int asl_smooth_robust_sequences_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                                  const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                                  const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                                  double huber_px, int max_iters, void *d_out, void *d_results, void *d_cov, void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {K, dist, n_dist, tag_size}, d_seed, nullptr, seq_start, n_seq,
                                    sigma_px, sigma_rot, sigma_trans, huber_px, max_iters, d_out, d_results, d_cov, d_cov != nullptr, true}, stream);
}

extern "C" int asl_smooth_robust_sequences_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                                 const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                                                 const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                                 double huber_px, int max_iters, asl_cam_pose *out, asl_smooth_result *results, asl_pose_cov *cov)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {K, dist, n_dist, tag_size}, seed, nullptr, seq_start, n_seq,
                            sigma_px, sigma_rot, sigma_trans, huber_px, max_iters, out, results, cov, cov != nullptr, true});
}

extern "C" int asl_smooth_timed_sequences_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                                 const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                                 const double *d_times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                                 double sigma_trans, double huber, int max_iters, void *d_out, void *d_results, void *d_cov,
                                                 void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {K, dist, n_dist, tag_size}, d_seed, d_times, seq_start, n_seq,
                                    sigma_px, sigma_rot, sigma_trans, huber, max_iters, d_out, d_results, d_cov, d_cov != nullptr, true}, stream);
}

extern "C" int asl_smooth_timed_sequences_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                                const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                                                const double *times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                                double sigma_trans, double huber, int max_iters, asl_cam_pose *out, asl_smooth_result *results,
                                                asl_pose_cov *cov)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {K, dist, n_dist, tag_size}, seed, times, seq_start, n_seq,
                            sigma_px, sigma_rot, sigma_trans, huber, max_iters, out, results, cov, cov != nullptr, true});
}

extern "C" int asl_smooth_rig_sequences_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                               int n_ids, const void *d_rig, double tag_size, const void *d_seed, const double *d_frame_times,
                                               const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                               double rig_huber_px, int max_iters, void *d_out, void *d_results, void *d_cov, void *stream)
{
    return smooth_frames_device(d, {d_obs, n_frames, max_tags, d_map, n_ids, {nullptr, nullptr, 0, tag_size}, d_seed, d_frame_times, seq_start, n_seq,
                                    sigma_px, sigma_rot, sigma_trans, rig_huber_px, max_iters, d_out, d_results, d_cov, d_cov != nullptr, true,
                                    n_cams, d_rig}, stream);
}

extern "C" int asl_smooth_rig_sequences_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                                              int n_ids, const asl_rig_camera *rig, double tag_size, const asl_cam_pose *seed,
                                              const double *frame_times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                              double sigma_trans, double rig_huber_px, int max_iters, asl_cam_pose *out, asl_smooth_result *results,
                                              asl_pose_cov *cov)
{
    return smooth_batch(d, {obs, n_frames, max_tags, map, n_ids, {nullptr, nullptr, 0, tag_size}, seed, frame_times, seq_start, n_seq,
                            sigma_px, sigma_rot, sigma_trans, rig_huber_px, max_iters, out, results, cov, cov != nullptr, true, n_cams, rig});
}

// ---- locating unmapped tags from posed frames (k_locate.inc)

static_assert(sizeof(TagFitRec) == sizeof(asl_tag_fit) && sizeof(asl_tag_fit) == 40, "asl_tag_fit layout");

// One locate call, whichever of the four entry points made it, in their argument order; cov may be NULL: not asked for.
// The single-camera forms leave n_cams 0 and rig NULL; the rig forms give n_cams and the table and leave cam's K and dist
// NULL, n_dist 0.  obs, poses, map (in / out), rig, fit and cov are all host (*_batch) or all device pointers.
struct LocateCall {
    const void *obs; int n_cams, n_frames, max_tags;
    const void *poses;
    void *map; int n_ids;
    const void *rig; Camera cam;
    double gate; int min_views; double sigma_px;
    void *fit, *cov;
};

static bool is_rig(const LocateCall &c) { return c.n_cams || c.rig; }

// Every refusal, before anything is written or enqueued.  A rig's table is checked last, as check_localize_call does: where
// it is, or (device) in a copy read back.
static int check_locate_call(const asl_detector *d, const LocateCall &c, bool device)
{
    const bool rig = is_rig(c);
    if (!d) return fail(ASL_EINVAL, "NULL detector");
    if (!c.obs || !c.poses || !c.map || !(rig ? c.rig : (const void *)c.cam.K) || !c.fit) return fail(ASL_EINVAL, "NULL argument");
    if (c.n_frames < 0) return fail(ASL_EINVAL, "n_frames < 0");
    if (rig && (c.n_cams < 1 || c.n_cams > RIG_MAX_CAMS)) return fail(ASL_EINVAL, "n_cams must be in [1, %d] (got %d)", RIG_MAX_CAMS, c.n_cams);
    if (int rc = check_obs_args(c.max_tags, c.n_ids, c.cam)) return rc;
    if (rig && c.n_cams * c.max_tags > RIG_MAX_SLOTS)
        return fail(ASL_EINVAL, "n_cams * max_tags must be <= %d (got %d x %d)", RIG_MAX_SLOTS, c.n_cams, c.max_tags);
    if ((size_t)(rig ? c.n_cams : 1) * (size_t)c.n_frames * (size_t)c.max_tags > 0x7fffffffull)
        return fail(ASL_EINVAL, "the block must hold fewer than 2^31 records (got %d x %d x %d)", rig ? c.n_cams : 1, c.n_frames, c.max_tags);
    if (!(c.gate >= 0) || !std::isfinite(c.gate)) return fail(ASL_EINVAL, "max_view_rms_px must be >= 0 (got %g)", c.gate);
    if (c.min_views < 1) return fail(ASL_EINVAL, "min_views must be >= 1 (got %d)", c.min_views);
    if (int rc = check_sigma_px(c.sigma_px)) return rc;
    if (!rig) return ASL_OK;
    asl_rig_camera tab[RIG_MAX_CAMS];
    if (device) {
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipMemcpy(tab, c.rig, sizeof(asl_rig_camera) * (size_t)c.n_cams, hipMemcpyDeviceToHost));
    }
    return check_rig_table(device ? tab : (const asl_rig_camera *)c.rig, c.n_cams);
}

// c's pointers are the device's.  The workspace (per-id marks, counts and offsets, the view list over every record of the
// block) is carved from d->locate_ws before the first launch; the four kernels follow each other on the stream without a
// host wait.  One camera is a block of n_cams = 1.
static int launch_locate(asl_detector *d, const LocateCall &c, hipStream_t st)
{
    static const double no_K[9] = {};
    const bool rig = is_rig(c);
    const int n_cams = rig ? c.n_cams : 1;
    const size_t ni = (size_t)c.n_ids, nsl = (size_t)n_cams * (size_t)c.n_frames * (size_t)c.max_tags;
    LocateArgs a{};
    if (carve_ws(d->locate_ws, [&](WsCarve &w) {
            a.seen = w.take<int>(ni); a.cnt = w.take<int>(ni); a.ptr = w.take<int>(ni + 1); a.views = w.take<int>(std::max<size_t>(nsl, 1));
        }))
        return fail(ASL_ENOMEM, "tag location workspace allocation failed");
    a.obs = (const ObsRec *)c.obs; a.n_cams = n_cams; a.n_frames = c.n_frames; a.max_tags = c.max_tags; a.poses = (const CamPoseRec *)c.poses;
    a.map = (MapTagRec *)c.map; a.n_ids = c.n_ids;
    const CamDev cam = make_cam(d, rig ? no_K : c.cam.K, c.cam.dist, c.cam.n_dist, c.cam.tag_size);   // a rig: for its half alone
    const RigCamRec *tab = (const RigCamRec *)c.rig;
    TagFitRec *fit = (TagFitRec *)c.fit;
    PoseCovRec *cov = (PoseCovRec *)c.cov;
    const dim3 ids((unsigned int)c.n_ids), wave(ASL_WAVE);
    HIPCHK(hipMemsetAsync(a.seen, 0, sizeof(int) * ni, st));
    if (nsl) hipLaunchKernelGGL(k_locate_mark, dim3((unsigned int)((nsl + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_locate_count, ids, wave, 0, st, a);
    hipLaunchKernelGGL(k_locate_scan, dim3(1), dim3(MAP_WG), 0, st, a);
    if (!rig && cov)
        hipLaunchKernelGGL(k_locate_solve<true>, ids, wave, 0, st, a, cam, c.gate, c.min_views, fit, cov, c.sigma_px);
    else if (!rig)
        hipLaunchKernelGGL(k_locate_solve<false>, ids, wave, 0, st, a, cam, c.gate, c.min_views, fit, cov, c.sigma_px);
    else if (cov)
        hipLaunchKernelGGL(k_locate_solve_rig<true>, ids, wave, 0, st, a, tab, cam.half, c.gate, c.min_views, fit, cov, c.sigma_px);
    else
        hipLaunchKernelGGL(k_locate_solve_rig<false>, ids, wave, 0, st, a, tab, cam.half, c.gate, c.min_views, fit, cov, c.sigma_px);
    HIPCHK(hipGetLastError());
    return ASL_OK;
}

// the host forms: the map goes in and comes back through solve_out, the frame poses and a rig's table are staged there too
static int locate_batch(asl_detector *d, const LocateCall &c)
{
    if (int rc = check_locate_call(d, c, false)) return rc;
    const bool rig = is_rig(c);
    const size_t ni = (size_t)c.n_ids, pose_bytes = sizeof(asl_cam_pose) * (size_t)c.n_frames, rig_bytes = sizeof(asl_rig_camera) * (size_t)c.n_cams;
    OutPiece o[] = {{c.map, sizeof(asl_map_tag) * ni}, {c.fit, sizeof(asl_tag_fit) * ni}, {c.cov, c.cov ? sizeof(asl_pose_cov) * ni : 0},
                    {nullptr, pose_bytes}, {nullptr, rig_bytes}};
    if (int rc = stage_host_call(d, "tag location", o, c.obs, (rig ? c.n_cams : 1) * c.n_frames, c.max_tags, nullptr, c.n_ids)) return rc;
    HIPCHK(hipMemcpy(o[0].dev, c.map, o[0].bytes, hipMemcpyHostToDevice));
    if (pose_bytes) HIPCHK(hipMemcpy(o[3].dev, c.poses, pose_bytes, hipMemcpyHostToDevice));
    if (rig) HIPCHK(hipMemcpy(o[4].dev, c.rig, rig_bytes, hipMemcpyHostToDevice));
    LocateCall dc = c;
    dc.obs = d->loc_obs.p ? (const void *)d->loc_obs.p : c.obs;  // no frame: never read, but not NULL
    dc.poses = o[3].dev ? o[3].dev : c.poses;
    dc.map = o[0].dev; dc.fit = o[1].dev; dc.cov = o[2].dev; dc.rig = o[4].dev;
    if (int rc = launch_locate(d, dc, nullptr)) return rc;
    return fetch_out(o);
}

static constexpr auto locate_frames_device = frames_device<LocateCall, check_locate_call, launch_locate>;   // the two device forms

extern "C" int asl_locate_tags_frames_device(asl_detector *d, const void *d_obs, int n_frames, int max_tags, const void *d_poses, void *d_map,
                                             int n_ids, const double *K, const double *dist, int n_dist, double tag_size, double max_view_rms_px,
                                             int min_views, double sigma_px, void *d_fit, void *d_cov, void *stream)
{
    return locate_frames_device(
        d, {d_obs, 0, n_frames, max_tags, d_poses, d_map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_view_rms_px, min_views, sigma_px, d_fit, d_cov},
        stream);
}

extern "C" int asl_locate_tags_batch(asl_detector *d, const asl_obs *obs, int n_frames, int max_tags, const asl_cam_pose *poses, asl_map_tag *map,
                                     int n_ids, const double *K, const double *dist, int n_dist, double tag_size, double max_view_rms_px,
                                     int min_views, double sigma_px, asl_tag_fit *fit, asl_pose_cov *cov)
{
    return locate_batch(d, {obs, 0, n_frames, max_tags, poses, map, n_ids, nullptr, {K, dist, n_dist, tag_size}, max_view_rms_px, min_views, sigma_px, fit, cov});
}

extern "C" int asl_locate_tags_rig_frames_device(asl_detector *d, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_poses,
                                                 void *d_map, int n_ids, const void *d_rig, double tag_size, double max_view_rms_px, int min_views,
                                                 double sigma_px, void *d_fit, void *d_cov, void *stream)
{
    return locate_frames_device(
        d, {d_obs, n_cams, n_frames, max_tags, d_poses, d_map, n_ids, d_rig, {nullptr, nullptr, 0, tag_size}, max_view_rms_px, min_views, sigma_px, d_fit, d_cov},
        stream);
}

extern "C" int asl_locate_tags_rig_batch(asl_detector *d, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_cam_pose *poses,
                                         asl_map_tag *map, int n_ids, const asl_rig_camera *rig, double tag_size, double max_view_rms_px,
                                         int min_views, double sigma_px, asl_tag_fit *fit, asl_pose_cov *cov)
{
    return locate_batch(d, {obs, n_cams, n_frames, max_tags, poses, map, n_ids, rig, {nullptr, nullptr, 0, tag_size}, max_view_rms_px, min_views, sigma_px, fit, cov});
}
