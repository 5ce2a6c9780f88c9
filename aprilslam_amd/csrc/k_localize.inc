// Multi-tag camera localisation against a known tag map (asl_localize_frames_device / asl_localize_batch).
// One wavefront per frame, float64 throughout.  The frame's max_tags slots x 4 corners are spread over the 64 lanes
// (corner c = 4 * slot + q on lane c % 64); every pass over the corners ends in a butterfly sum over the wave
// (butterfly_sum, k_wave.inc: every lane then holds the same bits), so the small serial parts (candidate choice, 6x6
// Cholesky, the step) run redundantly in all lanes on identical inputs, without a broadcast.
//   gather  taking-part slots (flags & 1, mapped id) -> world corners (LDS, double) and image corners (LDS, float32 as packed);
//           a map entry with a size of its own has its corners at that size, the others at the call's tag_size (map_tag_half)
//   seed    <= 8 seeding slots (flags & 2) of largest corner area; each slot's PnP pose (solved at the call's tag_size: a
//           sized slot's translation times h_id / half, which is its pose at its own size) and its mirrored planar minimum,
//           composed with the map, scored over ALL taking-part corners: reseed_poses' camera half with the tags held fixed
//   refine  Levenberg-Marquardt on camera<-world, T <- [Rod(w) | v] T, 10 trial steps at most
//   gate    optional: while the slot of largest own 4-corner RMS exceeds max_tag_rms_px it is dropped and the solve runs
//           again (one slot at a time, at most 8)
//   cov     k_localize<true> only (asl_localize_cov_*): one more linearisation at the pose written, then lane c solves column c
//           of sigma^2 (J^T J)^-1 in the output convention (pose_cov_column_dev, k_pnp.inc; tests/pose_cov_ref.py)
//   mapcov  k_localize_mapcov only (asl_localize_mapcov_*): the map's joint covariance carried into that covariance
//           (loc_map_term; tests/localize_mapcov_ref.py)
//   bundles asl_localize_bundles_*: the grid's second dimension chooses one of several maps (the tag layouts of several
//           objects), one wavefront per (frame, bundle), each the solve above against its own table (loc_bundle_map)
// tests/localize_ref.py is the NumPy statement of the same computation.  Latency-bound scalar float64 like k_pnp.inc:
// the time goes into the dependent chains of the passes and reductions, not into bytes (136 B per slot in, 160 B per frame out).
// These steps are written once, in loc_solve_frame<COV, Model>, over the slots of a model: where slot g's record lives,
// how one of its corners is projected, and how its camera<-world candidate becomes the pose solved for.  LocOneCam (here)
// is one camera's max_tags slots and makes k_localize; LocRig (k_rig.inc) is the n_cams * max_tags global slots of a rig
// and makes k_localize_rig.  Each kernel is its set-up, a model and one call.

struct MapTagRec {  // == asl_map_tag, 104 bytes
    double T[12];   // rows 0..2 of world<-tag
    int32_t valid;
    float size;     // the tag's own side; 0: the call's tag_size
};

// The half side of map entry e, the one rule of every solver that takes a map.  hid comes in as the call's half and stays
// that for size 0; a size of its own makes it (double)(size * 0.5f) (halving a float32 is exact: the float32 half the PnP
// would form).  False for an entry that does not take part: valid == 0, or a size that is negative or not finite.
__device__ __forceinline__ bool map_tag_half(const MapTagRec &e, double &hid)
{
    const float sz = e.size;
    if (sz > 0.0f) hid = (double)(sz * 0.5f);
    return e.valid && sz >= 0.0f && sz < INFINITY;
}

struct CamPoseRec {  // == asl_cam_pose, 160 bytes
    double T[16];
    double rms_px, rms_seed_px;
    int32_t n_tags, n_rejected, status, seed_slot;
};

#define LOC_MAX_SEEDS 8
#define LOC_LM_ITERS 10
#define LOC_MIRRORED 256
#define LOC_MAX_GATE_DROPS 8
#define LOC_Z_MIN 1e-9
#define LOC_BEHIND_COST 1e12

// (area, slot) with the larger area, the lower slot on a tie: the same pair in every lane afterwards
template <int J>
__device__ __forceinline__ void argmax_step(double &a, int &s)
{
    const double pa = __builtin_bit_cast(double, lane_xor<J>(__builtin_bit_cast(unsigned long long, a)));
    const int ps = (int)lane_xor32<J>((unsigned int)s);
    if (pa > a || (pa == a && ps < s)) { a = pa; s = ps; }
}

// Squared pixel error of one corner at camera point P = R X + t; with NE its rows of the Jacobian
// d uv / d delta = J_proj [-[P]x | I] are added to acc: JtJ (packed lower triangle, 21) and Jt r (6).
// (A template rather than a null pointer: a pointer chosen at run time keeps the arrays out of registers.)
// ROBUST (the sequence solve's Huber loss, k_smooth.inc; every other caller leaves it false and gets the code above alone):
// with s = |r| > hk the corner costs 2 hk s - hk^2 instead of s^2, its rows enter acc times wgt = hk / s, and *over is set;
// else wgt = 1 and the sums are the plain ones to the bit.  Lane-local: one sqrt, one division, 27 products.
template <bool NE, bool ROBUST = false>
__device__ __forceinline__ double loc_corner(const CamDev &c, const double *R, const double *t, const double *X, double iu, double iv,
                                             double *acc, double hk = 0.0, bool *over = nullptr)
{
    double P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    if (!(P[2] > LOC_Z_MIN)) return LOC_BEHIND_COST;
    project_dev(c, P, uv, NE ? Jp : nullptr);
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
        const double nPx[9] = {0, P[2], -P[1], -P[2], 0, P[0], P[1], -P[0], 0};  // -[P]x
        double J0[6], J1[6];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            J0[k] = Jp[0] * nPx[k] + Jp[1] * nPx[3 + k] + Jp[2] * nPx[6 + k];
            J0[3 + k] = Jp[k];
            J1[k] = Jp[3] * nPx[k] + Jp[4] * nPx[3 + k] + Jp[5] * nPx[6 + k];
            J1[3 + k] = Jp[3 + k];
        }
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
    if constexpr (ROBUST) return rho;
    else return r0 * r0 + r1 * r1;
}

// The slot model of one camera: slot s is record fo[s], every corner goes through cam, and the pose solved for is the
// camera's, so a slot's camera<-world candidate is written straight to where the caller wants it (no copy).
struct LocOneCam {
    const CamDev &cam;
    const ObsRec *fo;  // the frame's max_tags records
    int max_tags;
    __device__ __forceinline__ int nslots() const { return max_tags; }
    __device__ __forceinline__ const ObsRec *rec(int s) const { return fo + s; }
    template <bool NE, bool ROBUST = false>
    __device__ __forceinline__ double corner(int, const double *R, const double *t, const double *X, double iu, double iv, double *acc,
                                             double hk = 0.0, bool *over = nullptr) const
    {
        return loc_corner<NE, ROBUST>(cam, R, t, X, iu, iv, acc, hk, over);
    }
    // d uv / d Pb (2 x 3) of a corner of slot s at the body point Pb = R X + t, here the camera's own; false behind the camera
    __device__ __forceinline__ bool jac(int, const double *Pb, double *Jr) const
    {
        if (!(Pb[2] > LOC_Z_MIN)) return false;
        double uv[2];
        project_dev(cam, Pb, uv, Jr);
        return true;
    }
    // the solved pose (R, t) that slot s's PnP pose To and map tag M propose (loc_candidate)
    __device__ __forceinline__ void candidate(int, const double *To, const double *M, bool mirror, double *R, double *t) const;
    // camera<-world of slot s's camera at the solved pose (R, t): the pose itself
    __device__ __forceinline__ void camera_pose(int, const double *R, const double *t, double *Rc, double *tc) const
    {
#pragma unroll
        for (int i = 0; i < 9; i++) Rc[i] = R[i];
        tc[0] = t[0]; tc[1] = t[1]; tc[2] = t[2];
    }
};

// LDS of one frame (dynamic): world corners double[3 * n4], slot area double[max_tags], image corners float[2 * n4],
// slot state int[max_tags] (0 out, 1 taking part, 2 dropped by the gate)
struct LocLds {
    double *X, *area;
    float *uv;
    int *state;
};

__host__ __device__ constexpr size_t loc_lds_bytes(int max_tags)
{
    return (size_t)max_tags * (4 * 3 * sizeof(double) + 4 * 2 * sizeof(float) + sizeof(double) + sizeof(int));
}

__device__ __forceinline__ LocLds loc_lds(double *s_dyn, int max_tags)
{
    LocLds L;
    L.X = s_dyn;
    L.area = L.X + 12 * max_tags;
    L.uv = (float *)(L.area + max_tags);
    L.state = (int *)(L.uv + 8 * max_tags);
    return L;
}

// Shoelace area of a slot's 8 float corners, in this order of operations (tests/localize_ref.py: corner_area)
__device__ __forceinline__ double loc_area(const float *cf)
{
    const double x0 = cf[0], y0 = cf[1], x1 = cf[2], y1 = cf[3], x2 = cf[4], y2 = cf[5], x3 = cf[6], y3 = cf[7];
    const double a = (x0 * y1 - x1 * y0) + (x1 * y2 - x2 * y1) + (x2 * y3 - x3 * y2) + (x3 * y0 - x0 * y3);
    return 0.5 * fabs(a);
}

// Slot s into L: its 4 world corners (object corners +-half, lb rb rt lt, through the 3x4 world<-tag M) and 4 image corners
__device__ __forceinline__ void loc_gather_slot(const LocLds &L, int s, const double *M, double half, const float *cf)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double ox = (q == 1 || q == 2) ? half : -half, oy = (q >= 2) ? half : -half;
#pragma unroll
        for (int r = 0; r < 3; r++) L.X[3 * (4 * s + q) + r] = M[4 * r] * ox + M[4 * r + 1] * oy + M[4 * r + 3];
        L.uv[2 * (4 * s + q)] = cf[2 * q];
        L.uv[2 * (4 * s + q) + 1] = cf[2 * q + 1];
    }
}

// Gather of one frame's n slots against the map, slot s being the record rec(s): state 1 for a taking-part slot
// (flags & 1, mapped id: map_tag_half), its corners at the slot's own half, its area if seeds(flags), else -1.  Returns
// the number of taking-part slots and, with nseed, sets the number of seeding ones, both identical in every lane.
template <class Rec, class Seeds>
__device__ __forceinline__ int loc_gather(Rec rec, int n, const MapTagRec *map, int n_ids, double half, Seeds seeds, const LocLds &L, int lane,
                                          int *nseed = nullptr)
{
    int npart = 0, ns = 0;
    for (int s = lane; s < n; s += ASL_WAVE) {
        const ObsRec *r = rec(s);
        const int id = r->id, fl = r->flags;
        double hs = half;
        const bool part = (fl & 1) && id >= 0 && id < n_ids && map_tag_half(map[id], hs);
        L.state[s] = part ? 1 : 0;
        L.area[s] = -1.0;
        if (!part) continue;
        npart++;
        float cf[8];
#pragma unroll
        for (int k = 0; k < 8; k++) cf[k] = r->corners[k];
        loc_gather_slot(L, s, map[id].T, hs, cf);
        if (seeds(fl)) {
            ns++;
            L.area[s] = loc_area(cf);
        }
    }
    __syncthreads();
    if (nseed) *nseed = butterfly_sum<64>(ns);
    return butterfly_sum<64>(npart);
}

// The first K indices of [0, n) in the order (area descending, index ascending), counting only areas >= 0 (a negative or
// NaN area never takes part), identical in every lane: sel[0..nsel) in that order, 0x7fffffff after; returns nsel.  Each
// round takes the largest of what the earlier rounds left, so nothing is written and no barrier is needed.
template <int K, class Area>
__device__ __forceinline__ int loc_top_k(int n, int lane, Area area, int (&sel)[K])
{
    int nsel = 0, pp = -1;
    double pa = INFINITY;
#pragma unroll
    for (int r = 0; r < K; r++) {
        double ba = -1.0;
        int bs = 0x7fffffff;
        for (int i = lane; i < n; i += ASL_WAVE) {  // a lane's indices ascend: a tie keeps the lower one
            const double ar = area(i);
            if (ar > ba && (ar < pa || (ar == pa && i > pp))) { ba = ar; bs = i; }  // the second test: not taken already
        }
        argmax_step<1>(ba, bs); argmax_step<2>(ba, bs); argmax_step<4>(ba, bs);
        argmax_step<8>(ba, bs); argmax_step<16>(ba, bs); argmax_step<32>(ba, bs);
        sel[r] = ba >= 0 ? bs : 0x7fffffff;
        if (ba >= 0) { nsel++; pa = ba; pp = bs; }
    }
    return nsel;
}

// Every candidate of the chosen indices, in ascending index order, plain before mirrored: make(i) does index i's own work
// once and returns a callable cand(mirrored, P) that writes the candidate pose P (R row-major 9, t 3); score(P) is its
// cost.  A cost strictly below best replaces best and Pb; returns the code of the last replacement (index, + LOC_MIRRORED
// if mirrored), -1 if none.  For k_calib and k_map.  loc_solve_frame has the same loop written out, once for k_localize and
// k_localize_rig: through this helper k_localize measured 5 % slower (see there), and the two here are not that hot.
template <int K, class Make, class Score>
__device__ __forceinline__ int loc_best_candidate(const int (&sel)[K], int nsel, Make make, Score score, double &best, double *Pb)
{
    int code = -1, prev = -1;
    for (int j = 0; j < nsel; j++) {
        int i = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < K; r++)
            if (sel[r] > prev && sel[r] < i) i = sel[r];
        prev = i;
        const auto cand = make(i);
        for (int m = 0; m < 2; m++) {
            double P[12];
            cand(m == 1, P);
            const double c = score(P);
            if (c < best) {
                best = c;
                code = i + LOC_MIRRORED * m;
#pragma unroll
                for (int k = 0; k < 12; k++) Pb[k] = P[k];
            }
        }
    }
    return code;
}

// Total cost over the active corners (state == 1) of the model's slots, identical in every lane; with NE also the normal
// equations in ne.
// ROBUST: every corner through the Huber loss of threshold hk (the model's corner<NE, true>), and *soft the number of active
// slots with a corner over it.  A slot's corners are four neighbouring lanes of one round of the loop (64 is a multiple of 4),
// a rig's global slots as one camera's, so the slot's OR is two quad exchanges; every lane takes every round, for the
// exchanges to read live lanes.
template <bool NE, bool ROBUST = false, class Model>
__device__ __forceinline__ double loc_pass(const Model &m, const double *R, const double *t, const LocLds &L, int lane, double *ne,
                                           [[maybe_unused]] double hk = 0.0, [[maybe_unused]] int *soft = nullptr)
{
    const int n4 = 4 * m.nslots();
    double cost = 0, acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0;
    if constexpr (ROBUST) {
        int ns = 0;
        for (int base = 0; base < n4; base += ASL_WAVE) {
            const int k = base + lane;
            const bool act = k < n4 && L.state[k >> 2] == 1;
            bool over = false;
            if (act) cost += m.template corner<NE, true>(k >> 2, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], acc, hk, &over);
            unsigned int o = over ? 1u : 0u;
            o |= lane_xor32<1>(o);
            o |= lane_xor32<2>(o);
            ns += (o && (k & 3) == 0) ? 1 : 0;
        }
        *soft = butterfly_sum<64>(ns);
    } else {
        for (int k = lane; k < n4; k += ASL_WAVE) {
            if (L.state[k >> 2] != 1) continue;
            cost += m.template corner<NE>(k >> 2, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], acc);
        }
    }
    if constexpr (NE) {
#pragma unroll
        for (int i = 0; i < 27; i++) ne[i] = butterfly_sum<64>(acc[i]);
    }
    return butterfly_sum<64>(cost);
}

// The one-camera spelling, for k_calib and k_map: the n4 / 4 slots of camera c (no records: a pass reads LDS only)
template <bool NE>
__device__ __forceinline__ double loc_pass(const CamDev &c, const double *R, const double *t, const LocLds &L, int n4, int lane, double *ne)
{
    return loc_pass<NE>(LocOneCam{c, nullptr, n4 >> 2}, R, t, L, lane, ne);
}

// The fixed schedule (tests/localize_ref.py: lm) on a pose (R, t), refined in place by the left update R <- Rod(w) R,
// t <- Rod(w) t + v; returns the final cost.  pass(R, t, std::true_type{} / std::false_type{}, ne) returns the cost at
// (R, t), with true_type also the normal equations (packed lower triangle 21, then J^T r 6) in ne.
template <class Pass>
__device__ __forceinline__ double pose_lm(Pass pass, double *R, double *t)
{
    double ne[27];
    double cost = pass(R, t, std::true_type{}, ne);
    double lambda = 1e-3;
    for (int it = 0; it < LOC_LM_ITERS; it++) {
        double A[21], d[6];
#pragma unroll
        for (int i = 0; i < 21; i++) A[i] = ne[i];
#pragma unroll
        for (int a = 0; a < 6; a++) { A[TRI(a, a)] += lambda * ne[TRI(a, a)]; d[a] = -ne[21 + a]; }
        if (!chol6_solve_tri_dev(A, d)) { lambda *= 10; continue; }
        double dR[9], Rn[9], tn[3];
        rodrigues_dev(d, dR);
        mat3_mul_dev(dR, R, Rn);
#pragma unroll
        for (int r = 0; r < 3; r++) tn[r] = dR[3 * r] * t[0] + dR[3 * r + 1] * t[1] + dR[3 * r + 2] * t[2] + d[3 + r];
        const double cn = pass(Rn, tn, std::false_type{}, nullptr);
        if (cn < cost) {
            const bool stop = cost - cn < 1e-12 * cost;
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = Rn[i];
            t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
            cost = cn;
            lambda *= 0.1;
            if (stop) break;
            cost = pass(R, t, std::true_type{}, ne);
        } else
            lambda *= 10;
    }
    return cost;
}

// camera<-world of slot s's PnP pose (or its mirrored planar minimum, map_init.mirrored_pose) and map tag M: T_obs inv(M)
__device__ __forceinline__ void loc_candidate(const double *To, const double *M, bool mirror, double *R, double *t)
{
    double Ro[9], to[3] = {To[3], To[7], To[11]};
#pragma unroll
    for (int r = 0; r < 3; r++) { Ro[3 * r] = To[4 * r]; Ro[3 * r + 1] = To[4 * r + 1]; Ro[3 * r + 2] = To[4 * r + 2]; }
    if (mirror) {  // R' = (2 s s^T - I) R diag(-1, -1, 1), s = t / |t|
        const double n = sqrt(to[0] * to[0] + to[1] * to[1] + to[2] * to[2]);
        const double s[3] = {to[0] / n, to[1] / n, to[2] / n};
        double Rs[9], Rm[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Rs[3 * i + j] = 2.0 * s[i] * s[j] - (i == j ? 1.0 : 0.0);
        mat3_mul_dev(Rs, Ro, Rm);
#pragma unroll
        for (int r = 0; r < 3; r++) { Ro[3 * r] = -Rm[3 * r]; Ro[3 * r + 1] = -Rm[3 * r + 1]; Ro[3 * r + 2] = Rm[3 * r + 2]; }
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = Ro[3 * i] * M[4 * j] + Ro[3 * i + 1] * M[4 * j + 1] + Ro[3 * i + 2] * M[4 * j + 2];  // Ro Rm^T
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = to[i] - (R[3 * i] * M[3] + R[3 * i + 1] * M[7] + R[3 * i + 2] * M[11]);
}

__device__ __forceinline__ void LocOneCam::candidate(int, const double *To, const double *M, bool mirror, double *R, double *t) const
{
    loc_candidate(To, M, mirror, R, t);
}

// status 1 (no taking-part slot) / 2 (no candidate): identity pose, nothing used
__device__ __forceinline__ void loc_write_none(CamPoseRec *o, int status)
{
#pragma unroll
    for (int i = 0; i < 16; i++) o->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
    o->rms_px = 0; o->rms_seed_px = 0; o->n_tags = 0; o->n_rejected = 0; o->status = status; o->seed_slot = -1;
}

// status 1 of a frame's covariance (the frame has no pose): zeros, the sigma as given, by the lanes that store a solved one
__device__ __forceinline__ void loc_cov_write_none(PoseCovRec *oc, double sigma_px, int lane)
{
    if (lane < 36) oc->cov[lane] = 0.0;
    if (lane == 36) oc->sigma_px = sigma_px;
    if (lane == 37) { oc->dof = 0; oc->status = 1; }
}

// ---- the uncertainty of the map carried into the pose covariance (asl_localize_mapcov_*, asl_localize_rig_mapcov_*;
// tests/localize_mapcov_ref.py).  With J_s (8 x 6) the rows of slot s the solver forms, Jr [-[Pb]x | I] at the body point
// Pb = R X + t, and M_s (8 x 6) the same residuals' rows over the tag's (omega, v), a left update of world<-tag in the
// world frame: (Jr R) [-[X]x | I], a first-order error e of the map moves the pose by -A^-1 sum_s N_s e_j(s), A = sum
// J_s^T J_s, N_s = J_s^T M_s.  So C = sigma^2 A^-1 + A^-1 Q A^-1 with Q = sum_{s, s'} N_s Sigma[j(s), j(s')] N_s'^T over the
// active slots whose tag has a block in the map's joint covariance (asl_mapcov_*'s d_cov_slot, d_map_cov); a tag
// without one is exact.
enum { LOC_COV_NONE = 0, LOC_COV_PIXEL = 1, LOC_COV_MAP = 2 };  // loc_solve_frame's COV

struct LocMapCov {  // what asl_mapcov_* wrote: the matrix (row-major, leading dimension ld = 6 * cap_tags), the block of every id
    const double *cov;
    const int *slot;
    int ld;
};

#define LOC_MAPCOV_PITCH 37  /* doubles per slot of a round in LDS: 36, and odd so that the lanes' rows spread over the banks */

// N_s = J_s^T M_s (row-major 6 x 6) of active slot s at the pose (R, t), from the corners in LDS; a corner behind its camera
// adds no row, as in loc_corner
template <class Model>
__device__ __forceinline__ void loc_slot_cross(const Model &m, const LocLds &L, int s, const double *R, const double *t, double *N)
{
#pragma unroll
    for (int i = 0; i < 36; i++) N[i] = 0;
    for (int q = 0; q < 4; q++) {
        const double *X = L.X + 3 * (4 * s + q);
        double Pb[3], Jr[6];
#pragma unroll
        for (int r = 0; r < 3; r++) Pb[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
        if (!m.jac(s, Pb, Jr)) continue;
#pragma unroll
        for (int row = 0; row < 2; row++) {
            const double *j = Jr + 3 * row;
            double a[3];  // j R: d uv / d X
#pragma unroll
            for (int k = 0; k < 3; k++) a[k] = j[0] * R[k] + j[1] * R[3 + k] + j[2] * R[6 + k];
            const double Jc[6] = {Pb[1] * j[2] - Pb[2] * j[1], Pb[2] * j[0] - Pb[0] * j[2], Pb[0] * j[1] - Pb[1] * j[0], j[0], j[1], j[2]};
            const double Mc[6] = {X[1] * a[2] - X[2] * a[1], X[2] * a[0] - X[0] * a[2], X[0] * a[1] - X[1] * a[0], a[0], a[1], a[2]};
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) N[6 * i + k] += Jc[i] * Mc[k];
        }
    }
}

// The block of the lane's slot of round r (slot 64 r + lane): -1 for a slot that is not active or whose tag has no block,
// and *bad set for an entry outside [-1, ld / 6)
template <class Model>
__device__ __forceinline__ int loc_slot_block(const Model &m, const LocLds &L, const LocMapCov &mc, int s, bool *bad)
{
    if (s >= m.nslots() || L.state[s] != 1) return -1;
    const int k = mc.slot[m.rec(s)->id];
    if (k < -1 || k >= mc.ld / 6) { *bad = true; return -1; }
    return k;
}

// E = G Q G^T (6 x 6 into sE, LDS, both triangles from one computation) with G = Amap A^-1 the map from the slots' pulls to
// the output convention (Amap = diag(-R^T, -R^T), pose_cov_column_dev<true>'s) and A the packed J^T J in ne.  The pair sum:
// the slots go by rounds of 64, one slot a lane.  For each pair of rounds (ra, rb) the lanes put their round-rb slot's N
// and block into LDS, and every lane adds, for its own round-ra slot a and the 64 slots b of the round in lane order,
// N_a Sigma[j(a), j(b)] N_b^T to its own lower triangle of Q; the lanes' triangles are then summed by butterfly_sum.  Every
// order is fixed: the same input gives the same bytes.  256 active slots are 4 x 4 round pairs of 64 x 64 pairs.
// Returns the number of slots that contribute (the same in every lane); *bad: a slot entry out of range or a Sigma entry
// that is not finite.  A must be positive definite (the caller's pd).
template <class Model>
__device__ __forceinline__ int loc_map_term(const Model &m, const LocLds &L, const double *R, const double *t, const double *ne, const LocMapCov &mc,
                                            int lane, double *sE, bool *bad_out)
{
    __shared__ double sN[ASL_WAVE * LOC_MAPCOV_PITCH];
    __shared__ int sK[ASL_WAVE];
    const int rounds = (m.nslots() + ASL_WAVE - 1) / ASL_WAVE;
    double Q[21];
#pragma unroll
    for (int i = 0; i < 21; i++) Q[i] = 0;
    bool bad = false;
    int nq = 0;
    for (int ra = 0; ra < rounds; ra++) {
        double Na[36];
        const int a = ASL_WAVE * ra + lane, ka = loc_slot_block(m, L, mc, a, &bad);
        if (ka >= 0) { loc_slot_cross(m, L, a, R, t, Na); nq++; }
        for (int rb = 0; rb < rounds; rb++) {
            {
                double Nb[36];
                const int b = ASL_WAVE * rb + lane, kb = loc_slot_block(m, L, mc, b, &bad);
                if (kb >= 0) {
                    loc_slot_cross(m, L, b, R, t, Nb);
#pragma unroll
                    for (int i = 0; i < 36; i++) sN[lane * LOC_MAPCOV_PITCH + i] = Nb[i];
                }
                sK[lane] = kb;
            }
            __syncthreads();
            for (int l2 = 0; l2 < ASL_WAVE; l2++) {
                const int kb = sK[l2];  // the same in every lane
                if (kb < 0 || ka < 0) continue;
                const double *Nb = sN + l2 * LOC_MAPCOV_PITCH, *S = mc.cov + (size_t)6 * ka * mc.ld + 6 * kb;
                double T[36];  // N_a Sigma_ab
#pragma unroll
                for (int i = 0; i < 36; i++) T[i] = 0;
#pragma unroll
                for (int k = 0; k < 6; k++)
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const double v = S[(size_t)k * mc.ld + j];
                        bad = bad || !isfinite(v);
#pragma unroll
                        for (int i = 0; i < 6; i++) T[6 * i + j] += Na[6 * i + k] * v;
                    }
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j <= i; j++) {
                        double s = 0;
#pragma unroll
                        for (int k = 0; k < 6; k++) s += T[6 * i + k] * Nb[6 * j + k];
                        Q[TRI(i, j)] += s;
                    }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 21; i++) Q[i] = butterfly_sum<64>(Q[i]);
    nq = butterfly_sum<64>(nq);
    *bad_out = butterfly_sum<64>(bad ? 1 : 0) != 0;
    // G = Amap A^-1, column c of A^-1 from one solve (identical in every lane)
    double G[36];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double A[21], x[6];
#pragma unroll
        for (int i = 0; i < 21; i++) A[i] = ne[i];
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = i == c ? 1.0 : 0.0;
        chol6_solve_tri_dev(A, x);
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 3; i++) G[6 * (3 * b + i) + c] = -(R[i] * x[3 * b] + R[3 + i] * x[3 * b + 1] + R[6 + i] * x[3 * b + 2]);
    }
    double U[36];  // G Q
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) s += G[6 * r + i] * Q[i >= j ? TRI(i, j) : TRI(j, i)];
            U[6 * r + j] = s;
        }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c <= r; c++) {
                double s = 0;
#pragma unroll
                for (int j = 0; j < 6; j++) s += U[6 * r + j] * G[6 * c + j];
                sE[6 * r + c] = s;
                sE[6 * c + r] = s;
            }
    }
    __syncthreads();
    return nq;
}

// One frame's solve over the slots of model m, steps 1 to 6 of the header, by one wavefront: the pose solved for (the
// camera's, or the rig's) goes to o as world<-body.  COV: also the first-order covariance of the pose written (asl_pose_cov)
// into oc, scaled by sigma_px or, for 0, by the solve's own cost / dof.  The plain instantiation never touches oc and sigma_px.
// COV == LOC_COV_MAP (mc given): the map's uncertainty is added to it (loc_map_term); with no contributing slot the record is
// the LOC_COV_PIXEL one to the byte, and a bad slot entry or block gives status 3, zeros, the pose as it is.
template <int COV, class Model>
__device__ __forceinline__ void loc_solve_frame(const Model &m, const LocLds &L, const MapTagRec *__restrict__ map, int n_ids, double half,
                                                double gate, CamPoseRec *o, PoseCovRec *oc, double sigma_px, int lane,
                                                [[maybe_unused]] const LocMapCov &mc = LocMapCov{})
{
    const int n = m.nslots();
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return loc_pass<decltype(ne_tag)::value>(m, R, t, L, lane, ne);
    };

    // 1: gather (its barrier also publishes what the caller put into LDS before: the rig's camera table)
    int nseed;
    const int npart = loc_gather([&](int s) { return m.rec(s); }, n, map, n_ids, half, [](int fl) { return (fl & 2) != 0; }, L, lane, &nseed);
    if (npart == 0 || nseed == 0) {
        if (lane == 0) loc_write_none(o, npart == 0 ? 1 : 2);
        if constexpr (COV != LOC_COV_NONE) loc_cov_write_none(oc, sigma_px, lane);
        return;
    }

    // 2: the seeding slots of largest area (ties: lower slot), then every candidate in slot order, plain before mirrored
    int sel[LOC_MAX_SEEDS];
    const int nsel = loc_top_k(n, lane, [&](int s) { return L.area[s]; }, sel);
    // loc_best_candidate's loop, written out: through the helper k_localize measured 5 % slower (tools/localize_lab.py,
    // interleaved runs; about 2 % when the winner is rebuilt instead of copied), with the same instructions but for the
    // copy of the best pose and the layout.  This is the one written-out copy, for both kernels; a change to the candidate
    // rule goes here and into loc_best_candidate.
    double R[9], t[3], best = INFINITY;
    int code = -1, prev = -1;
    for (int j = 0; j < nsel; j++) {
        int s = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < LOC_MAX_SEEDS; r++)
            if (sel[r] > prev && sel[r] < s) s = sel[r];
        prev = s;
        const ObsRec *fo = m.rec(s);
        double To[12], M[12];
        const double *Mp = map[fo->id].T;
#pragma unroll
        for (int k = 0; k < 12; k++) { To[k] = fo->T[k]; M[k] = Mp[k]; }
        // a sized tag: the PnP solved it at the call's half, so the rotation holds and the translation is short by
        // half / h_id (object and translation scaled together leave every ray where it is, under any lens)
        const float sz = map[fo->id].size;
        if (sz > 0.0f) {
            const double k = (double)(sz * 0.5f) / half;
            To[3] *= k; To[7] *= k; To[11] *= k;
        }
        for (int mi = 0; mi < 2; mi++) {
            double Rc[9], tc[3];
            m.candidate(s, To, M, mi == 1, Rc, tc);
            const double cc = pass(Rc, tc, std::false_type{}, nullptr);
            if (cc < best) {
                best = cc;
                code = s + LOC_MIRRORED * mi;
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rc[i];
                t[0] = tc[0]; t[1] = tc[1]; t[2] = tc[2];
            }
        }
    }
    if (code < 0) {  // every candidate scored NaN
        if (lane == 0) loc_write_none(o, 2);
        if constexpr (COV != LOC_COV_NONE) loc_cov_write_none(oc, sigma_px, lane);
        return;
    }

    // 3: refine
    double cost = pose_lm(pass, R, t);

    // 4: the gate, one slot at a time: the worst slot over the gate goes, and the solve runs again from the current pose
    int nused = npart, nrej = 0;
    if (gate > 0) {
        for (int round = 0; round < LOC_MAX_GATE_DROPS && nused > 1; round++) {
            double wr = -1.0;
            int ws = 0x7fffffff;
            for (int s = lane; s < n; s += ASL_WAVE) {
                if (L.state[s] != 1) continue;
                double e[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = 4 * s + q;
                    e[q] = m.template corner<false>(s, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], nullptr);
                }
                const double rms = sqrt(((e[0] + e[1]) + (e[2] + e[3])) / 4);
                if (rms > wr) { wr = rms; ws = s; }
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

    // 5: world<-body = inv(body<-world)
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

    // 6: the covariance at the pose just written: one more linearisation over the corners still in LDS, then lane c
    // solves column c (every lane holds the same J^T J after the butterfly sums; lanes past 5 repeat column 5 and store nothing)
    if constexpr (COV != LOC_COV_NONE) {
        double ne[27], col[6], sig;
        const double c1 = loc_pass<true>(m, R, t, L, lane, ne);
        const int dof = 8 * nused - 6;
        const double s2 = pose_cov_sigma2(sigma_px, c1, dof, &sig);
        const int c = lane < 6 ? lane : 5;
        const bool pd = pose_cov_column_dev<true>(ne, R, t, c, col) && isfinite(s2);
        if constexpr (COV == LOC_COV_MAP) {
            // 7: the map's share.  Without a contributing slot the column is stored as above, to the byte
            __shared__ double sE[36];
            bool bad = false;
            const int nq = pd ? loc_map_term(m, L, R, t, ne, mc, lane, sE, &bad) : 0;
            if (lane < 6) {
                if (bad || !pd || nq == 0)
                    pose_cov_store_column(oc, c, col, s2, pd && !bad);
                else {
#pragma unroll
                    for (int r = 0; r < 6; r++) {
                        if (r < c) continue;
                        const double v = s2 * col[r] + sE[6 * r + c];
                        oc->cov[6 * r + c] = v;
                        oc->cov[6 * c + r] = v;
                    }
                }
            }
            if (lane == 36) oc->sigma_px = sig;
            if (lane == 37) { oc->dof = dof; oc->status = !pd ? 2 : bad ? 3 : 0; }
        } else {
            if (lane < 6) pose_cov_store_column(oc, c, col, s2, pd);
            if (lane == 36) oc->sigma_px = sig;
            if (lane == 37) { oc->dof = dof; oc->status = pd ? 0 : 2; }
        }
    }
}

// The bundle dimension of k_localize and k_localize_rig (asl_localize_bundles_*): the grid is (frame, bundle), and wavefront
// (f, b) solves frame f against table b of map (gridDim.y tables of n_ids entries, bundle<-tag) into record f * gridDim.y + b.
// The one-map entry points launch gridDim.y = 1: table 0, record f.
__device__ __forceinline__ const MapTagRec *loc_bundle_map(const MapTagRec *map, int n_ids) { return map + (size_t)blockIdx.y * (size_t)n_ids; }
__device__ __forceinline__ size_t loc_bundle_record() { return (size_t)blockIdx.x * gridDim.y + blockIdx.y; }

// One wavefront per (frame, bundle); COV: also cov[record] (world<-camera), which the plain instantiation never touches
template <bool COV>
__global__ void __launch_bounds__(64) k_localize(const ObsRec *__restrict__ obs, int max_tags, const MapTagRec *__restrict__ map, int n_ids,
                                                 CamDev cam, double gate, CamPoseRec *__restrict__ out, PoseCovRec *__restrict__ cov,
                                                 double sigma_px)
{
    extern __shared__ double s_dyn[];
    const LocOneCam m{cam, obs + (size_t)blockIdx.x * max_tags, max_tags};
    const size_t rec = loc_bundle_record();
    loc_solve_frame<COV>(m, loc_lds(s_dyn, max_tags), loc_bundle_map(map, n_ids), n_ids, cam.half, gate, out + rec, COV ? cov + rec : nullptr,
                         sigma_px, (int)threadIdx.x);
}

// k_localize<true> with the map's joint covariance carried into cov[frame] (asl_localize_mapcov_*): loc_solve_frame's
// LOC_COV_MAP mode, a kernel of its own, so that the two above keep their arguments and their code
__global__ void __launch_bounds__(64) k_localize_mapcov(const ObsRec *__restrict__ obs, int max_tags, const MapTagRec *__restrict__ map, int n_ids,
                                                        CamDev cam, double gate, CamPoseRec *__restrict__ out, PoseCovRec *__restrict__ cov,
                                                        double sigma_px, LocMapCov mc)
{
    extern __shared__ double s_dyn[];
    const LocOneCam m{cam, obs + (size_t)blockIdx.x * max_tags, max_tags};
    loc_solve_frame<LOC_COV_MAP>(m, loc_lds(s_dyn, max_tags), map, n_ids, cam.half, gate, out + blockIdx.x, cov + blockIdx.x, sigma_px,
                                 (int)threadIdx.x, mc);
}
