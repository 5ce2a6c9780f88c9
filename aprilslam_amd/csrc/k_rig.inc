// Multi-camera rig localisation against a known tag map (asl_localize_rig_frames_device / asl_localize_rig_batch).
// k_localize.inc's solve with one unknown pose rig<-world (R, t) per frame and n_cams cameras rigidly mounted on the rig:
// camera c has its own pinhole + lens model and a fixed mounting E_c = camera_c<-rig.  A world corner X seen by camera c:
//   P_r = R X + t,  P_c = Re_c P_r + te_c,  residual project_c(P_c) - (iu, iv)
// and, with the left update (R, t) <- (Rod(w) R, Rod(w) t + v), d uv / d (w, v) = J_proj_c(P_c) Re_c [-[P_r]x | I]:
// loc_corner's rows with J_proj Re_c for J_proj and the cross-product matrix at P_r.
// One wavefront per frame, float64 throughout, every sum a wave butterfly (the same input gives the same bytes).  The
// block is camera-major, obs[n_cams][n_frames][max_tags] (what all_gather_into_tensor makes of the ranks' packed blocks);
// a frame's n_cams * max_tags records are its global slots g = c * max_tags + s, spread over the lanes exactly as
// k_localize spreads one camera's slots, so gather, seed, refine, gate and covariance are its steps over global slots:
//   gather  as k_localize; the camera table (model, Re, te: RIG_CAM_DOUBLES per camera) goes to LDS first
//   seed    the <= 8 global slots with flags & 2 of largest corner area (pixels squared as they are: cameras of
//           different focal length are not put on one scale); a candidate of camera c is inv(E_c) (T_obs inv(map[id])),
//           scored over ALL taking-part corners of ALL cameras
//   refine, gate, cov   pose_lm / the gate loop / pose_cov_column_dev on rig<-world; the covariance is that of the
//           world<-rig pose written, the mountings and the map taken as exact
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

// loc_corner for a corner of the camera whose LDS record is cl: squared pixel error at rig point P_r = R X + t, with NE
// its two Jacobian rows J_proj Re [-[P_r]x | I] added to acc (JtJ packed lower triangle 21, Jt r 6).  The mounting is read
// from LDS where it is used: a per-camera choice among register copies would be a run-time-indexed array, i.e. scratch.
template <bool NE>
__device__ __forceinline__ double rig_corner(const double *cl, const double *R, const double *t, const double *X, double iu, double iv, double *acc)
{
    const double *Re = cl + 9, *te = cl + 18;
    double Pr[3], P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) Pr[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = Re[3 * r] * Pr[0] + Re[3 * r + 1] * Pr[1] + Re[3 * r + 2] * Pr[2] + te[r];
    if (!(P[2] > LOC_Z_MIN)) return LOC_BEHIND_COST;
    CamDev c;
    c.fx = cl[0]; c.fy = cl[1]; c.cx = cl[2]; c.cy = cl[3]; c.k1 = cl[4]; c.k2 = cl[5]; c.p1 = cl[6]; c.p2 = cl[7]; c.k3 = cl[8];
    c.half = 0; c.both_minima = 0; c.pad = 0;
    project_dev(c, P, uv, NE ? Jp : nullptr);
    const double r0 = uv[0] - iu, r1 = uv[1] - iv;
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
#pragma unroll
        for (int a = 0; a < 6; a++) {
            acc[21 + a] += J0[a] * r0 + J1[a] * r1;
#pragma unroll
            for (int b = 0; b <= a; b++) acc[TRI(a, b)] += J0[a] * J0[b] + J1[a] * J1[b];
        }
    }
    return r0 * r0 + r1 * r1;
}

// loc_pass over the global slots: total cost over the active corners (state == 1) of every camera, identical in every
// lane; with NE also the normal equations in ne
template <bool NE>
__device__ __forceinline__ double rig_pass(const double *cams, unsigned int magic, const double *R, const double *t, const LocLds &L, int n4, int lane,
                                           double *ne)
{
    double cost = 0, acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0;
    for (int k = lane; k < n4; k += ASL_WAVE) {
        if (L.state[k >> 2] != 1) continue;
        cost += rig_corner<NE>(cams + RIG_CAM_DOUBLES * rig_cam_of(k >> 2, magic), R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], acc);
    }
    if constexpr (NE) {
#pragma unroll
        for (int i = 0; i < 27; i++) ne[i] = butterfly_sum<64>(acc[i]);
    }
    return butterfly_sum<64>(cost);
}

// COV: also the first-order covariance of the world<-rig pose written (asl_pose_cov) into cov[frame], as k_localize<true>
template <bool COV>
__global__ void __launch_bounds__(64) k_localize_rig(const ObsRec *__restrict__ obs, int n_cams, int max_tags, const MapTagRec *__restrict__ map,
                                                     int n_ids, const RigCamRec *__restrict__ rig, double half, double gate,
                                                     CamPoseRec *__restrict__ out, PoseCovRec *__restrict__ cov, double sigma_px)
{
    extern __shared__ double s_dyn[];
    const int G = n_cams * max_tags, n4 = 4 * G, lane = threadIdx.x, n_frames = gridDim.x;
    const unsigned int magic = 65536u / (unsigned int)max_tags + 1u;
    double *cams = s_dyn;
    const LocLds L = loc_lds(s_dyn + RIG_CAM_DOUBLES * n_cams, G);
    CamPoseRec *o = out + blockIdx.x;
    // global slot g of this frame: camera g / max_tags, that camera's slot g % max_tags
    auto rec_of = [&](int g) -> const ObsRec * {
        const int c = rig_cam_of(g, magic);
        return obs + ((size_t)c * n_frames + blockIdx.x) * max_tags + (g - c * max_tags);
    };
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return rig_pass<decltype(ne_tag)::value>(cams, magic, R, t, L, n4, lane, ne);
    };

    // 0: the camera table: entry i of camera c (the lens coefficients past n_dist are zero whatever the record holds)
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

    // 1: gather (loc_gather over the global slots; its barrier also publishes the camera table)
    int npart = 0, nseed = 0;
    for (int g = lane; g < G; g += ASL_WAVE) {
        const ObsRec *r = rec_of(g);
        const int id = r->id, fl = r->flags;
        const bool part = (fl & 1) && id >= 0 && id < n_ids && map[id].valid;
        L.state[g] = part ? 1 : 0;
        L.area[g] = -1.0;
        if (!part) continue;
        npart++;
        float cf[8];
#pragma unroll
        for (int k = 0; k < 8; k++) cf[k] = r->corners[k];
        loc_gather_slot(L, g, map[id].T, half, cf);
        if (fl & 2) {
            nseed++;
            L.area[g] = loc_area(cf);
        }
    }
    __syncthreads();
    nseed = butterfly_sum<64>(nseed);
    npart = butterfly_sum<64>(npart);
    if (npart == 0 || nseed == 0) {
        if (lane == 0) loc_write_none(o, npart == 0 ? 1 : 2);
        if constexpr (COV) loc_cov_write_none(cov + blockIdx.x, sigma_px, lane);
        return;
    }

    // 2: the seeding global slots of largest area (ties: lower slot), then every candidate in slot order, plain before
    // mirrored (k_localize's loop: see there why it is written out)
    int sel[LOC_MAX_SEEDS];
    const int nsel = loc_top_k(G, lane, [&](int g) { return L.area[g]; }, sel);
    double R[9], t[3], best = INFINITY;
    int code = -1, prev = -1;
    for (int j = 0; j < nsel; j++) {
        int g = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < LOC_MAX_SEEDS; r++)
            if (sel[r] > prev && sel[r] < g) g = sel[r];
        prev = g;
        const ObsRec *fo = rec_of(g);
        const double *cl = cams + RIG_CAM_DOUBLES * rig_cam_of(g, magic), *Re = cl + 9, *te = cl + 18;
        double To[12], M[12];
        const double *Mp = map[fo->id].T;
#pragma unroll
        for (int k = 0; k < 12; k++) { To[k] = fo->T[k]; M[k] = Mp[k]; }
        for (int m = 0; m < 2; m++) {
            double Rk[9], tk[3], Rc[9], tc[3];
            loc_candidate(To, M, m == 1, Rk, tk);  // camera<-world; rig<-world = inv(E) of it: Re^T Rk, Re^T (tk - te)
            const double dk[3] = {tk[0] - te[0], tk[1] - te[1], tk[2] - te[2]};
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int k = 0; k < 3; k++) Rc[3 * i + k] = Re[i] * Rk[k] + Re[3 + i] * Rk[3 + k] + Re[6 + i] * Rk[6 + k];
                tc[i] = Re[i] * dk[0] + Re[3 + i] * dk[1] + Re[6 + i] * dk[2];
            }
            const double cc = pass(Rc, tc, std::false_type{}, nullptr);
            if (cc < best) {
                best = cc;
                code = g + LOC_MIRRORED * m;
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rc[i];
                t[0] = tc[0]; t[1] = tc[1]; t[2] = tc[2];
            }
        }
    }
    if (code < 0) {  // every candidate scored NaN
        if (lane == 0) loc_write_none(o, 2);
        if constexpr (COV) loc_cov_write_none(cov + blockIdx.x, sigma_px, lane);
        return;
    }

    // 3: refine
    double cost = pose_lm(pass, R, t);

    // 4: the gate over global slots, one at a time
    int nused = npart, nrej = 0;
    if (gate > 0) {
        for (int round = 0; round < LOC_MAX_GATE_DROPS && nused > 1; round++) {
            double wr = -1.0;
            int ws = 0x7fffffff;
            for (int g = lane; g < G; g += ASL_WAVE) {
                if (L.state[g] != 1) continue;
                const double *cl = cams + RIG_CAM_DOUBLES * rig_cam_of(g, magic);
                double e[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = 4 * g + q;
                    e[q] = rig_corner<false>(cl, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], nullptr);
                }
                const double rms = sqrt(((e[0] + e[1]) + (e[2] + e[3])) / 4);
                if (rms > wr) { wr = rms; ws = g; }
            }
            argmax_step<1>(wr, ws); argmax_step<2>(wr, ws); argmax_step<4>(wr, ws);
            argmax_step<8>(wr, ws); argmax_step<16>(wr, ws); argmax_step<32>(wr, ws);
            if (!(wr > gate)) break;
            __syncthreads();
            if (lane == 0) L.state[ws] = 2;
            __syncthreads();
            nrej++;
            nused--;
            cost = pose_lm(pass, R, t);
        }
    }

    // 5: world<-rig = inv(rig<-world)
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
            o->T[4 * r] = R[r]; o->T[4 * r + 1] = R[3 + r]; o->T[4 * r + 2] = R[6 + r];
            o->T[4 * r + 3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
        }
        o->T[12] = 0; o->T[13] = 0; o->T[14] = 0; o->T[15] = 1;
        o->rms_px = sqrt(cost / (4.0 * nused));
        o->rms_seed_px = sqrt(best / (4.0 * npart));
        o->n_tags = nused;
        o->n_rejected = nrej;
        o->status = 0;
        o->seed_slot = code;
    }

    // 6: the covariance at the pose just written, as k_localize<true> step 6
    if constexpr (COV) {
        PoseCovRec *oc = cov + blockIdx.x;
        double ne[27], col[6], sig;
        const double c1 = rig_pass<true>(cams, magic, R, t, L, n4, lane, ne);
        const int dof = 8 * nused - 6;
        const double s2 = pose_cov_sigma2(sigma_px, c1, dof, &sig);
        const int c = lane < 6 ? lane : 5;
        const bool pd = pose_cov_column_dev<true>(ne, R, t, c, col) && isfinite(s2);
        if (lane < 6) pose_cov_store_column(oc, c, col, s2, pd);
        if (lane == 36) oc->sigma_px = sig;
        if (lane == 37) { oc->dof = dof; oc->status = pd ? 0 : 2; }
    }
}
