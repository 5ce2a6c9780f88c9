// Multi-camera rig localisation against a known tag map (asl_localize_rig_frames_device / asl_localize_rig_batch).
// k_localize.inc's solve with one unknown pose rig<-world (R, t) per frame and n_cams cameras rigidly mounted on the rig:
// camera c has its own pinhole + lens model and a fixed mounting E_c = camera_c<-rig.  A world corner X seen by camera c:
//   P_r = R X + t,  P_c = Re_c P_r + te_c,  residual project_c(P_c) - (iu, iv)
// and, with the left update (R, t) <- (Rod(w) R, Rod(w) t + v), d uv / d (w, v) = J_proj_c(P_c) Re_c [-[P_r]x | I]:
// loc_corner's rows with J_proj Re_c for J_proj and the cross-product matrix at P_r.
// One wavefront per frame, float64 throughout, every sum a wave butterfly (the same input gives the same bytes).  The
// block is camera-major, obs[n_cams][n_frames][max_tags] (what all_gather_into_tensor makes of the ranks' packed blocks);
// a frame's n_cams * max_tags records are its global slots g = c * max_tags + s, spread over the lanes exactly as
// k_localize spreads one camera's slots.  The solve is k_localize.inc's loc_solve_frame, the one copy of gather, seed,
// refine, gate and covariance, over the slot model LocRig below; the kernel fills the camera table and calls it:
//   table   model, Re, te (RIG_CAM_DOUBLES per camera) to LDS first; the gather's barrier publishes it
//   seed    the <= 8 global slots with flags & 2 of largest corner area (pixels squared as they are: cameras of
//           different focal length are not put on one scale); a candidate of camera c is inv(E_c) (T_obs inv(map[id])),
//           scored over ALL taking-part corners of ALL cameras
//   cov     that of the world<-rig pose written, the mountings and the map taken as exact
// A rig of one camera with E_0 = I is k_localize: Re = I multiplies exactly.  tests/rig_ref.py is the NumPy statement.

struct RigCamRec {  // == asl_rig_camera, 216 bytes
    double K[9], dist[5], E[12];
    int32_t n_dist, reserved;
};

// a camera in LDS: fx fy cx cy k1 k2 p1 p2 k3 | Re (row-major 9) | te (3)
#define RIG_CAM_DOUBLES 21
#define RIG_MAX_CAMS 16
#define RIG_MAX_SLOTS 256

// dynamic LDS of one frame: the camera table, then k_localize's arrays over the n_cams * max_tags global slots
__host__ __device__ constexpr size_t rig_lds_bytes(int n_cams, int max_tags)
{
    return (size_t)n_cams * RIG_CAM_DOUBLES * sizeof(double) + loc_lds_bytes(n_cams * max_tags);
}

// g / max_tags for a global slot g < 256 and max_tags <= 256 by one multiplication: magic = 65536 / max_tags + 1 errs by
// less than g * max_tags / 65536 < 1 / max_tags, which no quotient's fraction part comes within of the next integer
__device__ __forceinline__ int rig_cam_of(int g, unsigned int magic) { return (int)(((unsigned int)g * magic) >> 16); }

// the projection model of the camera whose LDS record is cl
__device__ __forceinline__ CamDev rig_cam_dev(const double *cl)
{
    CamDev c;
    c.fx = cl[0]; c.fy = cl[1]; c.cx = cl[2]; c.cy = cl[3]; c.k1 = cl[4]; c.k2 = cl[5]; c.p1 = cl[6]; c.p2 = cl[7]; c.k3 = cl[8];
    c.half = 0; c.both_minima = 0; c.pad = 0;
    return c;
}

// loc_corner for a corner of the camera whose LDS record is cl: squared pixel error at rig point P_r = R X + t, with NE
// its two Jacobian rows J_proj Re [-[P_r]x | I] added to acc (JtJ packed lower triangle 21, Jt r 6).  The mounting is read
// from LDS where it is used: a per-camera choice among register copies would be a run-time-indexed array, i.e. scratch.
// ROBUST (the rig sequence solve's Huber loss, k_smooth.inc): loc_corner<NE, true>'s rho, wgt and *over on the same
// residual, the weight on the same 27 sums; every other caller leaves it false and gets the code above alone.
// MOUNT (the mounting calibration, k_rigcal.inc; with NE): nothing is summed; acc receives the corner's rows themselves,
// J0 J1 (6 + 6) as above, then the rows over the mounting's own left update (Re, te) <- (Rod(w) Re, Rod(w) te + v),
// J_proj [-[P_c]x | I] (6 + 6), then the residual (2): RIG_ROWS doubles.  A corner behind the camera leaves acc as it was.
#define RIG_ROWS 26
template <bool NE, bool ROBUST = false, bool MOUNT = false>
__device__ __forceinline__ double rig_corner(const double *cl, const double *R, const double *t, const double *X, double iu, double iv, double *acc,
                                             double hk = 0.0, bool *over = nullptr)
{
    const double *Re = cl + 9, *te = cl + 18;
    double Pr[3], P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) Pr[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = Re[3 * r] * Pr[0] + Re[3 * r + 1] * Pr[1] + Re[3 * r + 2] * Pr[2] + te[r];
    if (!(P[2] > LOC_Z_MIN)) return LOC_BEHIND_COST;
    project_dev(rig_cam_dev(cl), P, uv, NE ? Jp : nullptr);
    const double r0 = uv[0] - iu, r1 = uv[1] - iv;
    [[maybe_unused]] double wgt = 1.0, rho = 0.0;
    if constexpr (ROBUST) {
        const double e = r0 * r0 + r1 * r1, s = sqrt(e);
        const bool o = s > hk;
        wgt = o ? hk / s : 1.0;
        rho = o ? 2.0 * hk * s - hk * hk : e;
        *over = o;
    }
    if constexpr (NE) {
        double Jr[6];  // J_proj Re
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Jr[k] = Jp[0] * Re[k] + Jp[1] * Re[3 + k] + Jp[2] * Re[6 + k];
            Jr[3 + k] = Jp[3] * Re[k] + Jp[4] * Re[3 + k] + Jp[5] * Re[6 + k];
        }
        const double nPx[9] = {0, Pr[2], -Pr[1], -Pr[2], 0, Pr[0], Pr[1], -Pr[0], 0};  // -[P_r]x
        double J0[6], J1[6];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            J0[k] = Jr[0] * nPx[k] + Jr[1] * nPx[3 + k] + Jr[2] * nPx[6 + k];
            J0[3 + k] = Jr[k];
            J1[k] = Jr[3] * nPx[k] + Jr[4] * nPx[3 + k] + Jr[5] * nPx[6 + k];
            J1[3 + k] = Jr[3 + k];
        }
        if constexpr (MOUNT) {
            const double nPc[9] = {0, P[2], -P[1], -P[2], 0, P[0], P[1], -P[0], 0};  // -[P_c]x
#pragma unroll
            for (int k = 0; k < 3; k++) {
                acc[k] = J0[k]; acc[3 + k] = J0[3 + k]; acc[6 + k] = J1[k]; acc[9 + k] = J1[3 + k];
                acc[12 + k] = Jp[0] * nPc[k] + Jp[1] * nPc[3 + k] + Jp[2] * nPc[6 + k];
                acc[15 + k] = Jp[k];
                acc[18 + k] = Jp[3] * nPc[k] + Jp[4] * nPc[3 + k] + Jp[5] * nPc[6 + k];
                acc[21 + k] = Jp[3 + k];
            }
            acc[24] = r0; acc[25] = r1;
        } else {
#pragma unroll
            for (int a = 0; a < 6; a++) {
                if constexpr (ROBUST) acc[21 + a] += wgt * (J0[a] * r0 + J1[a] * r1);
                else acc[21 + a] += J0[a] * r0 + J1[a] * r1;
#pragma unroll
                for (int b = 0; b <= a; b++) {
                    if constexpr (ROBUST) acc[TRI(a, b)] += wgt * (J0[a] * J0[b] + J1[a] * J1[b]);
                    else acc[TRI(a, b)] += J0[a] * J0[b] + J1[a] * J1[b];
                }
            }
        }
    }
    if constexpr (ROBUST) return rho;
    else return r0 * r0 + r1 * r1;
}

// The slot model of a rig: global slot g is slot g % max_tags of camera g / max_tags in the camera-major block, its corners
// go through that camera's entry of the LDS table, and the pose solved for is rig<-world.
struct LocRig {
    const double *cams;  // LDS: RIG_CAM_DOUBLES per camera
    const ObsRec *obs;
    unsigned int magic;
    int n_cams, max_tags, n_frames, frame;
    __device__ __forceinline__ int nslots() const { return n_cams * max_tags; }
    __device__ __forceinline__ const double *cam_of(int g) const { return cams + RIG_CAM_DOUBLES * rig_cam_of(g, magic); }
    __device__ __forceinline__ const ObsRec *rec(int g) const
    {
        const int c = rig_cam_of(g, magic);
        return obs + ((size_t)c * n_frames + frame) * max_tags + (g - c * max_tags);
    }
    template <bool NE, bool ROBUST = false>
    __device__ __forceinline__ double corner(int g, const double *R, const double *t, const double *X, double iu, double iv, double *acc,
                                             double hk = 0.0, bool *over = nullptr) const
    {
        return rig_corner<NE, ROBUST>(cam_of(g), R, t, X, iu, iv, acc, hk, over);
    }
    // d uv / d Pb (2 x 3) of a corner of slot g at the rig point Pb = R X + t: J_proj Re of its camera; false behind it
    __device__ __forceinline__ bool jac(int g, const double *Pb, double *Jr) const
    {
        const double *cl = cam_of(g), *Re = cl + 9, *te = cl + 18;
        double P[3], uv[2], Jp[6];
#pragma unroll
        for (int r = 0; r < 3; r++) P[r] = Re[3 * r] * Pb[0] + Re[3 * r + 1] * Pb[1] + Re[3 * r + 2] * Pb[2] + te[r];
        if (!(P[2] > LOC_Z_MIN)) return false;
        project_dev(rig_cam_dev(cl), P, uv, Jp);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            Jr[k] = Jp[0] * Re[k] + Jp[1] * Re[3 + k] + Jp[2] * Re[6 + k];
            Jr[3 + k] = Jp[3] * Re[k] + Jp[4] * Re[3 + k] + Jp[5] * Re[6 + k];
        }
        return true;
    }
    // slot g's camera<-world candidate (loc_candidate) through its camera's mounting: rig<-world = inv(E) of it,
    // Re^T Rk, Re^T (tk - te)
    __device__ __forceinline__ void candidate(int g, const double *To, const double *M, bool mirror, double *R, double *t) const
    {
        const double *Re = cam_of(g) + 9, *te = cam_of(g) + 18;
        double Rk[9], tk[3];
        loc_candidate(To, M, mirror, Rk, tk);
        const double dk[3] = {tk[0] - te[0], tk[1] - te[1], tk[2] - te[2]};
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < 3; k++) R[3 * i + k] = Re[i] * Rk[k] + Re[3 + i] * Rk[3 + k] + Re[6 + i] * Rk[6 + k];
            t[i] = Re[i] * dk[0] + Re[3 + i] * dk[1] + Re[6 + i] * dk[2];
        }
    }
    // camera<-world of slot g's camera at the solved pose rig<-world = (R, t): E of it, Re R, Re t + te
    __device__ __forceinline__ void camera_pose(int g, const double *R, const double *t, double *Rc, double *tc) const
    {
        const double *Re = cam_of(g) + 9, *te = cam_of(g) + 18;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < 3; k++) Rc[3 * i + k] = Re[3 * i] * R[k] + Re[3 * i + 1] * R[3 + k] + Re[3 * i + 2] * R[6 + k];
            tc[i] = Re[3 * i] * t[0] + Re[3 * i + 1] * t[1] + Re[3 * i + 2] * t[2] + te[i];
        }
    }
};

// The camera table of a rig into LDS, by one wavefront: entry i of camera c (the lens coefficients past n_dist are zero
// whatever the record holds).  The caller's next barrier (loc_gather's) publishes it.
__device__ __forceinline__ void rig_fill_cams(double *cams, const RigCamRec *__restrict__ rig, int n_cams, int lane)
{
    for (int i = lane; i < RIG_CAM_DOUBLES * n_cams; i += ASL_WAVE) {
        const int c = i / RIG_CAM_DOUBLES, e = i - c * RIG_CAM_DOUBLES;
        const RigCamRec *rc = rig + c;
        double v;
        if (e < 4)
            v = rc->K[e == 0 ? 0 : e == 1 ? 4 : e == 2 ? 2 : 5];
        else if (e < 9)
            v = (e - 4 < 4 ? rc->n_dist >= 4 : rc->n_dist >= 5) ? rc->dist[e - 4] : 0.0;
        else if (e < 18)
            v = rc->E[4 * ((e - 9) / 3) + (e - 9) % 3];
        else
            v = rc->E[4 * (e - 18) + 3];
        cams[i] = v;
    }
}

// One wavefront per (frame, bundle) (loc_bundle_map, k_localize.inc); COV: also the first-order covariance of the world<-rig
// pose written (asl_pose_cov) into cov[record]
template <bool COV>
__global__ void __launch_bounds__(64) k_localize_rig(const ObsRec *__restrict__ obs, int n_cams, int max_tags, const MapTagRec *__restrict__ map,
                                                     int n_ids, const RigCamRec *__restrict__ rig, double half, double gate,
                                                     CamPoseRec *__restrict__ out, PoseCovRec *__restrict__ cov, double sigma_px)
{
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x;
    double *cams = s_dyn;

    rig_fill_cams(cams, rig, n_cams, lane);

    const LocRig m{cams, obs, 65536u / (unsigned int)max_tags + 1u, n_cams, max_tags, (int)gridDim.x, (int)blockIdx.x};
    const size_t rec = loc_bundle_record();
    loc_solve_frame<COV>(m, loc_lds(s_dyn + RIG_CAM_DOUBLES * n_cams, m.nslots()), loc_bundle_map(map, n_ids), n_ids, half, gate, out + rec,
                         COV ? cov + rec : nullptr, sigma_px, lane);
}

// k_localize_rig<true> with the map's joint covariance carried into cov[frame] (asl_localize_rig_mapcov_*), as k_localize_mapcov
__global__ void __launch_bounds__(64) k_localize_rig_mapcov(const ObsRec *__restrict__ obs, int n_cams, int max_tags, const MapTagRec *__restrict__ map,
                                                            int n_ids, const RigCamRec *__restrict__ rig, double half, double gate,
                                                            CamPoseRec *__restrict__ out, PoseCovRec *__restrict__ cov, double sigma_px, LocMapCov mc)
{
    extern __shared__ double s_dyn[];
    const int lane = threadIdx.x;
    double *cams = s_dyn;

    rig_fill_cams(cams, rig, n_cams, lane);

    const LocRig m{cams, obs, 65536u / (unsigned int)max_tags + 1u, n_cams, max_tags, (int)gridDim.x, (int)blockIdx.x};
    loc_solve_frame<LOC_COV_MAP>(m, loc_lds(s_dyn + RIG_CAM_DOUBLES * n_cams, m.nslots()), map, n_ids, half, gate, out + blockIdx.x, cov + blockIdx.x,
                                 sigma_px, lane, mc);
}
