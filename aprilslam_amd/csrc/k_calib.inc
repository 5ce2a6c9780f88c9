// Camera calibration from tag observations (asl_calibrate_frames_device / asl_calibrate_batch).
// theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) of the camera model of k_pnp.inc, shared by all frames, and one camera<-world
// pose per frame, float64 throughout; tests/calib_ref.py is the NumPy statement of the same computation.
//   k_calib_init    per frame (one wavefront): mapped slots, and the frame's share of the closed-form focal-length system
//                   (Zhang's two constraints per tag from its square -> quad homography, divided by |h1| |h2|)
//   k_calib_k0      one workgroup: the list of taking-part frames (>= 2 mapped slots), K0 (closed form or K_init)
//   k_calib_seed    per frame: planar pose of the <= 8 largest tags under K0 and its mirrored minimum, composed with the map
//                   and scored over all corners, pose-only LM (k_localize.inc: loc_candidate, loc_pass, pose_lm); then the
//                   frame's normal equations at (K0, no distortion, that pose)
//   k_calib_start   one workgroup: the list of used frames, the cost, lambda0
//   then max_iters times (joint Levenberg-Marquardt, the arrow-shaped normal equations reduced by the Schur complement):
//   k_calib_schur   per used frame: Cholesky of its damped 6x6 pose block U, U^-1 W, U^-1 g and its share of the
//                   reduced theta system V - W^T U^-1 W, g_theta - W^T U^-1 g_pose
//   k_calib_solve   one workgroup: the frames' shares summed, Cholesky of the reduced system -> d_theta, the trial theta
//   k_calib_step    per used frame: its pose step (back-substitution), the trial pose and its normal equations there
//   k_calib_decide  one workgroup: trial cost against the current one, lambda x0.1 / x10, accept (flip the buffers), stop
//   and once more k_calib_schur undamped, k_calib_finish (std from the reduced system's inverse, the records).
// lambda, the accepted state (cur: which of the two pose / normal-equation / theta buffers is current) and the stop flag
// live in device memory, so the whole solve is one submission; after the stop every kernel returns at once.  Sums over
// corners are butterfly sums over the wave (butterfly_sum, k_wave.inc), sums over frames run over the list of used frames in
// contiguous chunks of a fixed count, then over the chunks in order: no atomics, the same bytes on every run, and frames
// that do not take part change nothing.  Latency-bound like k_localize.inc: ~4 dependent launches per iteration.
//
// The lens is a compile-time parameter of the kernels that project (CAL_LENS_BROWN: the above, CamDev; CAL_LENS_FISHEYE:
// FishDev, the cv2.fisheye model of k_rectify.inc, theta = (fx, fy, cx, cy, k1, k2, k3, k4); tests/calib_fisheye_ref.py is
// its statement).  A fisheye has no closed-form focal length and no pinhole planar pose, so its K0 and seeds come from a
// focal ladder; k_calib_seed is replaced by three launches:
//   k_calib_fish_seed  one wavefront per (frame, rung): the frame seeded under the equidistant (f_j, f_j, centre) -- the
//                      <= 8 largest slots whose corners all lie within CAL_GATE rad of the axis, each slot's corner rays as
//                      pinhole coordinates through the same homography and planar pose, scored over all corners under the
//                      fisheye, pose-only LM -- its pose, cost and code per rung (one rung, K_init's, with K_init)
//   k_calib_fish_pick  one workgroup: every rung summed over the taking-part frames (cal_list_sum), the argmin, theta0, the
//                      winning rung's poses and seed records into place (or frame status 3)
//   k_calib_fish_lin   per frame: the normal equations at (K0, k = 0, that pose)
// k_calib_schur / solve / decide / finish read no lens; k_calib_step has it as a template parameter.

struct CalibResultRec {  // == asl_calib_result, 216 bytes
    double K[9], dist[5], std[9];
    double rms_px, rms_init_px;
    int32_t n_frames_used, n_corners, iterations, status;
};

struct CalibState {
    double theta[2][9];  // [cur] current, [1 - cur] trial
    double dtheta[9];
    double ratio, lambda, cost, seed_cost;
    int cur, done, solve_ok, status, iterations, n_used, n_corners, n_take;
};

#define CAL_HS 136   // doubles per frame of the augmented normal equations [J | r]^T [J | r] (packed lower triangle, <= 16 columns)
#define CAL_SB 64    // doubles per frame of the reduced system's share: S (packed, <= 45) at 0, b (<= 9) at 45
#define CAL_SB_B 45
#define CAL_BK 64    // doubles per frame of the back-substitution: U^-1 W (9 x 6) at 0, U^-1 g_pose (6) at 54
#define CAL_ZH 8     // doubles per frame of the closed form: pp pq qq pc qc ee ec rows
#define CAL_FR 4     // ints per frame: status (0, 1, 3), mapped slots, seed code, Schur ok
#define CAL_WG 1024  // threads of the single-workgroup kernels
#define CAL_CHUNKS (CAL_WG / 64)

struct CalibArgs {
    const ObsRec *obs;
    const MapTagRec *map;
    CalibState *st;
    int *list, *fr;
    double *zh, *seedc, *pose, *H, *SB, *back;
    CalibResultRec *res;
    CamPoseRec *out;
    double half, width, height, Kinit[4];
    int n_frames, max_tags, n_ids, n_dist, flags, has_init, np, max_iters;
    int sel[9];
    // the fisheye's focal ladder: rungs per frame (1 with K_init), and per (frame, rung) the seed pose (12), its cost and code
    int lens, n_rungs;
    double *lpose, *lcost;
    int *lcode;
};

#define CAL_LENS_BROWN 0
#define CAL_LENS_FISHEYE 1
#define CAL_RUNGS 13
#define CAL_GATE 1.3  // rad: a slot seeds only if the equidistant unprojection of all its corners lies within it

#define CAL_FIX_ASPECT 2

__device__ __forceinline__ int cal_nt(int n_dist) { return 11 + n_dist; }  // 6 pose + 4 + n_dist theta + residual

// Gather of one frame into LDS (k_localize.inc: loc_gather), every taking-part slot seeding; returns the number of
// taking-part slots (identical in every lane)
__device__ __forceinline__ int cal_gather(const CalibArgs &a, int f, int lane, const LocLds &L)
{
    const ObsRec *fo = a.obs + (size_t)f * a.max_tags;
    return loc_gather([=](int s) { return fo + s; }, a.max_tags, a.map, a.n_ids, a.half, [](int) { return true; }, L, lane);
}

// Homography (row-major 3x3) of the square (+-1, +-1), lb rb rt lt, onto the corners in x' = (u - cx) / s: the closed-form
// unit square -> quad mapping, composed with (X, Y) -> ((X + 1) / 2, (Y + 1) / 2)
template <class T>  // float: a record's corners; double: corner rays as pinhole coordinates
__device__ __forceinline__ void cal_square_h(const T *cf, double cx, double cy, double s, double *H)
{
    double x[4], y[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { x[q] = ((double)cf[2 * q] - cx) / s; y[q] = ((double)cf[2 * q + 1] - cy) / s; }
    const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], sx = (x[0] - x[1]) + (x[2] - x[3]);
    const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], sy = (y[0] - y[1]) + (y[2] - y[3]);
    const double den = dx1 * dy2 - dx2 * dy1;
    const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
    const double Hu[9] = {x[1] - x[0] + g * x[1], x[3] - x[0] + h * x[3], x[0],
                          y[1] - y[0] + g * y[1], y[3] - y[0] + h * y[3], y[0],
                          g, h, 1.0};
#pragma unroll
    for (int r = 0; r < 3; r++) {
        H[3 * r] = 0.5 * Hu[3 * r];
        H[3 * r + 1] = 0.5 * Hu[3 * r + 1];
        H[3 * r + 2] = 0.5 * Hu[3 * r] + 0.5 * Hu[3 * r + 1] + Hu[3 * r + 2];
    }
}

// camera<-tag [R | t] rows (12) of a tag whose square maps by H under focal lengths fx, fy (the same x' coordinates)
__device__ __forceinline__ void cal_planar_pose(const double *H, double fx, double fy, double s, double half, double *To)
{
    double Hn[9];
    const double sc[3] = {s / fx, s / fy, 1.0};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Hn[3 * r + c] = sc[r] * H[3 * r + c];
    const double n1 = sqrt(Hn[0] * Hn[0] + Hn[3] * Hn[3] + Hn[6] * Hn[6]), n2 = sqrt(Hn[1] * Hn[1] + Hn[4] * Hn[4] + Hn[7] * Hn[7]);
    double mu = (n1 + n2) / (2 * half);
    if (Hn[8] < 0) mu = -mu;
    double r1[3], r2[3], M[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) { r1[r] = Hn[3 * r] / (mu * half); r2[r] = Hn[3 * r + 1] / (mu * half); }
    const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
#pragma unroll
    for (int r = 0; r < 3; r++) { M[3 * r] = r1[r]; M[3 * r + 1] = r2[r]; M[3 * r + 2] = r3[r]; }
    nearest_rotation_dev(M, R);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        To[4 * r] = R[3 * r]; To[4 * r + 1] = R[3 * r + 1]; To[4 * r + 2] = R[3 * r + 2];
        To[4 * r + 3] = Hn[3 * r + 2] / mu;
    }
}

__device__ __forceinline__ CamDev cal_cam(const double *th, int n_dist, double half)
{
    CamDev c;
    c.fx = th[0]; c.fy = th[1]; c.cx = th[2]; c.cy = th[3];
    c.k1 = n_dist >= 4 ? th[4] : 0.0; c.k2 = n_dist >= 4 ? th[5] : 0.0;
    c.p1 = n_dist >= 4 ? th[6] : 0.0; c.p2 = n_dist >= 4 ? th[7] : 0.0;
    c.k3 = n_dist >= 5 ? th[8] : 0.0;
    c.half = half; c.both_minima = 0; c.pad = 0;
    return c;
}

// The two augmented rows [J | r] of one corner over (w, v, fx, fy, cx, cy, k1.., residual); false if it lies behind the camera
template <int NT>
__device__ __forceinline__ bool cal_rows(const CamDev &c, bool fix_aspect, double ratio, const double *R, const double *t, const double *X,
                                         double iu, double iv, double *J0, double *J1)
{
    double P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    if (!(P[2] > LOC_Z_MIN)) return false;
    project_dev(c, P, uv, Jp);
    const double nPx[9] = {0, P[2], -P[1], -P[2], 0, P[0], P[1], -P[0], 0};  // -[P]x
#pragma unroll
    for (int k = 0; k < 3; k++) {
        J0[k] = Jp[0] * nPx[k] + Jp[1] * nPx[3 + k] + Jp[2] * nPx[6 + k];
        J0[3 + k] = Jp[k];
        J1[k] = Jp[3] * nPx[k] + Jp[4] * nPx[3 + k] + Jp[5] * nPx[6 + k];
        J1[3 + k] = Jp[3 + k];
    }
    const double iz = 1 / P[2], x = P[0] * iz, y = P[1] * iz;
    const double r2 = x * x + y * y, r4 = r2 * r2;
    const double cd = 1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
    const double yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
    J0[6] = xd; J0[7] = fix_aspect ? ratio * xd : 0.0; J0[8] = 1.0; J0[9] = 0.0;
    J1[6] = 0.0; J1[7] = yd; J1[8] = 0.0; J1[9] = 1.0;
    if constexpr (NT >= 15) {
        J0[10] = c.fx * x * r2; J0[11] = c.fx * x * r4; J0[12] = c.fx * 2 * x * y; J0[13] = c.fx * (r2 + 2 * x * x);
        J1[10] = c.fy * y * r2; J1[11] = c.fy * y * r4; J1[12] = c.fy * (r2 + 2 * y * y); J1[13] = c.fy * 2 * x * y;
    }
    if constexpr (NT >= 16) { J0[14] = c.fx * x * (r4 * r2); J1[14] = c.fy * y * (r4 * r2); }
    J0[NT - 1] = uv[0] - iu;
    J1[NT - 1] = uv[1] - iv;
    return true;
}

// ---- the fisheye lens (CAL_LENS_FISHEYE)
struct FishDev {
    double fx, fy, cx, cy, k1, k2, k3, k4;
};

__device__ __forceinline__ FishDev cal_fish(const double *th, int n_dist)
{
    FishDev c;
    c.fx = th[0]; c.fy = th[1]; c.cx = th[2]; c.cy = th[3];
    c.k1 = n_dist >= 4 ? th[4] : 0.0; c.k2 = n_dist >= 4 ? th[5] : 0.0;
    c.k3 = n_dist >= 4 ? th[6] : 0.0; c.k4 = n_dist >= 4 ? th[7] : 0.0;
    return c;
}

struct FishPt {  // what the intrinsic columns of a corner's rows need
    double th, ex, ey, sx, sy;  // theta, (X / r, Y / r), (theta_d / r) (X, Y)
};

// A corner costs its pixel error unless it sits in the camera centre: no "behind the camera" under this lens
__device__ __forceinline__ bool fish_in_range(const double *P) { return (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2] > LOC_Z_MIN * LOC_Z_MIN; }

// Pixel of camera point P under the fisheye: theta = atan2(r, Z) by the arctangent the rectification is defined by
// (rectify_atan2_pos), theta_d = theta (1 + k1 theta^2 + ..), u = fx theta_d X / r + cx.  JAC: d uv / d P (2 x 3, row-major)
// into Jp and the intrinsic columns' terms into pt.  On the axis (r = 0, Z > 0) both are the finite limit: the direction
// (X / r, Y / r) counts as 0 and theta_d / r as 1 / Z, which leaves d u / d X = fx / Z, d v / d Y = fy / Z and zeros (the ray
// straight backwards, r = 0 with Z < 0, has no image: (cx, cy) and a zero Jacobian).
template <bool JAC>
__device__ __forceinline__ void project_fisheye_dev(const FishDev &c, const double *P, double *uv, double *Jp, FishPt *pt)
{
    const double X = P[0], Y = P[1], Z = P[2];
    const double rr = X * X + Y * Y, r = sqrt(rr);
    const double th = rectify_atan2_pos(r, Z), t2 = th * th;
    const double td = th * (1 + t2 * (c.k1 + t2 * (c.k2 + t2 * (c.k3 + t2 * c.k4))));
    const bool on = r == 0;
    const double ex = on ? 0.0 : X / r, ey = on ? 0.0 : Y / r;
    const double s = on ? (Z > 0 ? 1 / Z : 0.0) : td / r;
    uv[0] = c.fx * (s * X) + c.cx;
    uv[1] = c.fy * (s * Y) + c.cy;
    if constexpr (JAC) {
        const double dtd = 1 + t2 * (3 * c.k1 + t2 * (5 * c.k2 + t2 * (7 * c.k3 + t2 * 9 * c.k4)));
        const double rho2 = rr + Z * Z;
        const double a = on ? s : dtd * Z / rho2;  // d theta_d / d r at fixed Z
        const double b = -dtd * r / rho2;          // d theta_d / d Z at fixed r
        Jp[0] = c.fx * (a * ex * ex + s * (1 - ex * ex)); Jp[1] = c.fx * ((a - s) * ex * ey); Jp[2] = c.fx * (b * ex);
        Jp[3] = c.fy * ((a - s) * ex * ey); Jp[4] = c.fy * (a * ey * ey + s * (1 - ey * ey)); Jp[5] = c.fy * (b * ey);
        pt->th = th; pt->ex = ex; pt->ey = ey; pt->sx = s * X; pt->sy = s * Y;
    }
}

// The slot model of one fisheye camera for loc_pass (k_localize.inc): loc_corner's sums under this lens.  The shared bodies
// there stay Brown-only; this is the calibration's own pass.
struct CalFishCam {
    const FishDev &cam;
    int n;
    __device__ __forceinline__ int nslots() const { return n; }
    template <bool NE, bool ROBUST = false>
    __device__ __forceinline__ double corner(int, const double *R, const double *t, const double *X, double iu, double iv, double *acc,
                                             double = 0.0, bool * = nullptr) const
    {
        static_assert(!ROBUST, "the calibration has no robust loss");
        double P[3], uv[2];
        [[maybe_unused]] double Jp[6];
        [[maybe_unused]] FishPt pt;
#pragma unroll
        for (int r = 0; r < 3; r++) P[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
        if (!fish_in_range(P)) return LOC_BEHIND_COST;
        project_fisheye_dev<NE>(cam, P, uv, Jp, &pt);
        const double r0 = uv[0] - iu, r1 = uv[1] - iv;
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
                acc[21 + a] += J0[a] * r0 + J1[a] * r1;
#pragma unroll
                for (int b = 0; b <= a; b++) acc[TRI(a, b)] += J0[a] * J0[b] + J1[a] * J1[b];
            }
        }
        return r0 * r0 + r1 * r1;
    }
};

// cal_rows under the fisheye, over (w, v, fx, fy, cx, cy, k1, k2, k3, k4, residual): d u / d k_i = fx (X / r) theta^(2 i + 1);
// false if the corner sits in the camera centre
template <int NT>
__device__ __forceinline__ bool cal_rows(const FishDev &c, bool fix_aspect, double ratio, const double *R, const double *t, const double *X,
                                         double iu, double iv, double *J0, double *J1)
{
    static_assert(NT == 11 || NT == 15, "a fisheye has 0 or 4 coefficients");
    double P[3], uv[2], Jp[6];
    FishPt pt;
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + t[r];
    if (!fish_in_range(P)) return false;
    project_fisheye_dev<true>(c, P, uv, Jp, &pt);
    const double nPx[9] = {0, P[2], -P[1], -P[2], 0, P[0], P[1], -P[0], 0};  // -[P]x
#pragma unroll
    for (int k = 0; k < 3; k++) {
        J0[k] = Jp[0] * nPx[k] + Jp[1] * nPx[3 + k] + Jp[2] * nPx[6 + k];
        J0[3 + k] = Jp[k];
        J1[k] = Jp[3] * nPx[k] + Jp[4] * nPx[3 + k] + Jp[5] * nPx[6 + k];
        J1[3 + k] = Jp[3 + k];
    }
    J0[6] = pt.sx; J0[7] = fix_aspect ? ratio * pt.sx : 0.0; J0[8] = 1.0; J0[9] = 0.0;
    J1[6] = 0.0; J1[7] = pt.sy; J1[8] = 0.0; J1[9] = 1.0;
    if constexpr (NT >= 15) {
        const double t2 = pt.th * pt.th, p3 = pt.th * t2, p5 = p3 * t2, p7 = p5 * t2, p9 = p7 * t2;
        J0[10] = c.fx * pt.ex * p3; J0[11] = c.fx * pt.ex * p5; J0[12] = c.fx * pt.ex * p7; J0[13] = c.fx * pt.ex * p9;
        J1[10] = c.fy * pt.ey * p3; J1[11] = c.fy * pt.ey * p5; J1[12] = c.fy * pt.ey * p7; J1[13] = c.fy * pt.ey * p9;
    }
    J0[NT - 1] = uv[0] - iu;
    J1[NT - 1] = uv[1] - iv;
    return true;
}

// Entries [LO, HI) of the frame's packed augmented normal equations, summed over its corners and written to Hf.  The
// triangle is built in chunks so that the accumulators stay in registers (the corner's rows are recomputed per chunk).
template <int NT, int LO, int HI, class Cam>  // Cam: CamDev or FishDev, by cal_rows' overloads
__device__ __forceinline__ void cal_chunk(const Cam &c, bool fa, double ratio, const double *R, const double *t, const LocLds &L, int n4,
                                          int lane, double *Hf)
{
    constexpr int NTRI = NT * (NT + 1) / 2;
    double acc[HI - LO], behind = 0;
#pragma unroll
    for (int i = 0; i < HI - LO; i++) acc[i] = 0;
    for (int k = lane; k < n4; k += ASL_WAVE) {
        if (L.state[k >> 2] != 1) continue;
        double J0[NT], J1[NT];
        if (!cal_rows<NT>(c, fa, ratio, R, t, L.X + 3 * k, (double)L.uv[2 * k], (double)L.uv[2 * k + 1], J0, J1)) {
            behind += LOC_BEHIND_COST;
            continue;
        }
#pragma unroll
        for (int p = 0; p < NT; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) {
                const int idx = TRI(p, q);
                if (idx >= LO && idx < HI) acc[idx - LO] += J0[p] * J0[q] + J1[p] * J1[q];
            }
    }
#pragma unroll
    for (int i = 0; i < HI - LO; i++) {
        double v = butterfly_sum<64>(acc[i]);
        if (LO + i == NTRI - 1) v += butterfly_sum<64>(behind);  // the cost entry
        if (lane == ((LO + i) & (ASL_WAVE - 1))) Hf[LO + i] = v;
    }
}

template <int NT, class Cam>
__device__ __forceinline__ void cal_linearise(const Cam &c, bool fa, double ratio, const double *R, const double *t, const LocLds &L, int n4,
                                              int lane, double *Hf)
{
    constexpr int NTRI = NT * (NT + 1) / 2, C = (NTRI + 3) / 4;
    cal_chunk<NT, 0, C>(c, fa, ratio, R, t, L, n4, lane, Hf);
    cal_chunk<NT, C, 2 * C>(c, fa, ratio, R, t, L, n4, lane, Hf);
    cal_chunk<NT, 2 * C, 3 * C>(c, fa, ratio, R, t, L, n4, lane, Hf);
    cal_chunk<NT, 3 * C, NTRI>(c, fa, ratio, R, t, L, n4, lane, Hf);
}

// Sum over the list of frames of rows[f * stride + e] for e < ne, by a CAL_WG workgroup: CAL_CHUNKS contiguous chunks of the
// list, each summed in order, then the chunks in order, 64 entries of the row at a time.  The result lands in out (LDS) for
// every thread: ne rounded up to a multiple of 64 entries (64 for ne = 0), zero past ne.
__device__ __forceinline__ void cal_list_sum(const double *rows, int stride, int ne, const int *list, int n, double *s_part, double *out)
{
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int chunk = (n + CAL_CHUNKS - 1) / CAL_CHUNKS;
    for (int e0 = 0; e0 < max(ne, 1); e0 += 64) {
        const int e = e0 + lane;
        double acc = 0;
        if (e < ne) {
            const int k1 = min(n, (q + 1) * chunk);
            for (int k = q * chunk; k < k1; k++) acc += rows[(size_t)list[k] * stride + e];
        }
        s_part[q * 64 + lane] = acc;
        __syncthreads();
        if (threadIdx.x < 64) {
            double s = 0;
            for (int j = 0; j < CAL_CHUNKS; j++) s += s_part[j * 64 + threadIdx.x];
            out[e0 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// The frames f < n_frames for which take(f) holds, in frame order, into list, by a CAL_WG workgroup; returns their count
// (every thread); s_cnt: CAL_WG ints of LDS, count: an int of device memory for the count to pass through
template <class Take>
__device__ __forceinline__ int cal_make_list_of(int n_frames, Take take, int *list, int *s_cnt, int *count)
{
    const int tid = threadIdx.x, per = (n_frames + CAL_WG - 1) / CAL_WG;
    const int f0 = min(n_frames, tid * per), f1 = min(n_frames, f0 + per);
    int c = 0;
    for (int f = f0; f < f1; f++) c += take(f) ? 1 : 0;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < CAL_WG; i++) { const int v = s_cnt[i]; s_cnt[i] = run; run += v; }
        *count = run;
    }
    __syncthreads();
    int o = s_cnt[tid];
    for (int f = f0; f < f1; f++)
        if (take(f)) list[o++] = f;
    __syncthreads();
    const int n = *count;
    __syncthreads();
    return n;
}

// The frames whose fr status is 0 and that have >= 2 mapped slots (n_take: scratch for the count; the callers copy it where
// it belongs)
__device__ __forceinline__ int cal_make_list(const CalibArgs &a, int *s_cnt)
{
    return cal_make_list_of(a.n_frames, [&](int f) { return a.fr[CAL_FR * f] == 0 && a.fr[CAL_FR * f + 1] >= 2; }, a.list, s_cnt, &a.st->n_take);
}

// Cholesky solve of the packed n x n system A x = b in LDS (one thread); false if A is not positive definite
__device__ __forceinline__ bool cal_chol(double *A, double *b, int n)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            double s = A[TRI(i, j)];
            for (int k = 0; k < j; k++) s -= A[TRI(i, k)] * A[TRI(j, k)];
            if (i == j) {
                if (!(s > 0)) return false;
                A[TRI(i, i)] = sqrt(s);
            } else
                A[TRI(i, j)] = s / A[TRI(j, j)];
        }
    if (b) {
        for (int i = 0; i < n; i++) {
            double s = b[i];
            for (int k = 0; k < i; k++) s -= A[TRI(i, k)] * b[k];
            b[i] = s / A[TRI(i, i)];
        }
        for (int i = n - 1; i >= 0; i--) {
            double s = b[i];
            for (int k = i + 1; k < n; k++) s -= A[TRI(k, i)] * b[k];
            b[i] = s / A[TRI(i, i)];
        }
    }
    return true;
}

// ---- per frame: mapped slots and the closed-form partial sums
__global__ void __launch_bounds__(64) k_calib_init(CalibArgs a)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const ObsRec *fo = a.obs + (size_t)f * a.max_tags;
    const double cx = 0.5 * a.width, cy = 0.5 * a.height, s = 0.5 * (a.width + a.height);
    double acc[CAL_ZH];
#pragma unroll
    for (int i = 0; i < CAL_ZH; i++) acc[i] = 0;
    int npart = 0;
    for (int k = lane; k < a.max_tags; k += ASL_WAVE) {
        const int id = fo[k].id, fl = fo[k].flags;
        double hs = a.half;
        if (!((fl & 1) && id >= 0 && id < a.n_ids && map_tag_half(a.map[id], hs))) continue;
        npart++;
        if (a.has_init || a.lens != CAL_LENS_BROWN) continue;  // no closed form to feed
        float cf[8];
#pragma unroll
        for (int q = 0; q < 8; q++) cf[q] = fo[k].corners[q];
        double H[9];
        cal_square_h(cf, cx, cy, s, H);
        // Zhang's two constraints, divided by |h1| |h2|: every tag weighs the same, and a constraint the view does not
        // inform (h1^T B h2 of a fronto-parallel tag) stays at rounding level
        const double n = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]) * sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
        for (int m = 0; m < 2; m++) {
            double r[3];
#pragma unroll
            for (int i = 0; i < 3; i++) r[i] = m == 0 ? H[3 * i] * H[3 * i + 1] : H[3 * i] * H[3 * i] - H[3 * i + 1] * H[3 * i + 1];
#pragma unroll
            for (int i = 0; i < 3; i++) r[i] = n > 0 ? r[i] / n : 0.0;
            if (!(isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]))) continue;
            const double e = r[0] + r[1];  // fixed aspect ratio 1 (no K_init): a = b
            acc[0] += r[0] * r[0]; acc[1] += r[0] * r[1]; acc[2] += r[1] * r[1];
            acc[3] += r[0] * r[2]; acc[4] += r[1] * r[2];
            acc[5] += e * e; acc[6] += e * r[2]; acc[7] += 1.0;
        }
    }
    npart = butterfly_sum<64>(npart);
#pragma unroll
    for (int i = 0; i < CAL_ZH; i++) {
        const double v = butterfly_sum<64>(acc[i]);
        if (lane == i) a.zh[(size_t)CAL_ZH * f + i] = v;
    }
    if (lane == 0) {
        int *fr = a.fr + CAL_FR * f;
        fr[0] = npart >= 2 ? 0 : 1; fr[1] = npart; fr[2] = -1; fr[3] = 0;
        a.seedc[f] = 0.0;
    }
}

// ---- one workgroup: taking-part frames, K0
__global__ void __launch_bounds__(CAL_WG) k_calib_k0(CalibArgs a)
{
    __shared__ int s_cnt[CAL_WG];
    __shared__ double s_part[CAL_WG], s_sum[64];
    CalibState *st = a.st;
    const int n = cal_make_list(a, s_cnt);
    double th[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ratio = 1.0;
    int status = n == 0 ? 1 : 0;
    if (status == 0 && !a.has_init && a.lens == CAL_LENS_BROWN) {
        cal_list_sum(a.zh, CAL_ZH, CAL_ZH, a.list, n, s_part, s_sum);
        const double s = 0.5 * (a.width + a.height);
        const double pp = s_sum[0], pq = s_sum[1], qq = s_sum[2], pc = s_sum[3], qc = s_sum[4], ee = s_sum[5], ec = s_sum[6];
        double fa = NAN, fb = NAN;
        if (s_sum[7] > 0) {
            // ill-conditioned (the least eigenvalue per row, det / trace, not above 1e-6): fronto-parallel views inform only fx / fy
            const double m = s_sum[7];
            if (a.flags & CAL_FIX_ASPECT) {
                if (ee > 1e-6 * m) fb = -ec / ee;
                fa = fb;
            } else {
                const double det = pp * qq - pq * pq;
                if (det > 1e-6 * m * (pp + qq)) { fa = (-pc * qq + qc * pq) / det; fb = (-qc * pp + pc * pq) / det; }
            }
        }
        if (!(fa > 1e-6 && fb > 1e-6 && isfinite(fa) && isfinite(fb))) status = 2;
        else { th[0] = s / sqrt(fa); th[1] = s / sqrt(fb); th[2] = 0.5 * a.width; th[3] = 0.5 * a.height; }
    } else if (status == 0 && a.has_init) {  // (a fisheye without K_init: k_calib_fish_pick writes theta0)
        th[0] = a.Kinit[0]; th[1] = a.Kinit[1]; th[2] = a.Kinit[2]; th[3] = a.Kinit[3];
        ratio = a.Kinit[0] / a.Kinit[1];
    }
    if (a.flags & CAL_FIX_ASPECT) th[0] = ratio * th[1];
    if (threadIdx.x == 0) {
        for (int i = 0; i < 9; i++) { st->theta[0][i] = th[i]; st->theta[1][i] = th[i]; st->dtheta[i] = 0; }
        st->ratio = ratio; st->lambda = 1e-3; st->cost = 0; st->seed_cost = 0;
        st->cur = 0; st->done = status != 0; st->solve_ok = 0; st->status = status; st->iterations = 0;
        st->n_used = 0; st->n_corners = 0;
    }
}

// ---- per frame: seed pose under K0, then the frame's normal equations there
template <int ND>
__global__ void __launch_bounds__(64) k_calib_seed(CalibArgs a)
{
    constexpr int NT = 11 + ND;
    extern __shared__ double s_dyn[];
    const int f = blockIdx.x, lane = threadIdx.x, n4 = 4 * a.max_tags;
    if (a.st->status != 0 || a.fr[CAL_FR * f] != 0) return;
    const LocLds L = loc_lds(s_dyn, a.max_tags);
    cal_gather(a, f, lane, L);
    const ObsRec *fo = a.obs + (size_t)f * a.max_tags;
    double th[9];
#pragma unroll
    for (int i = 0; i < 9; i++) th[i] = a.st->theta[0][i];
    const CamDev cam0 = cal_cam(th, 0, a.half);
    const double s = 0.5 * (a.width + a.height);
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return loc_pass<decltype(ne_tag)::value>(cam0, R, t, L, n4, lane, ne);
    };

    // the <= 8 taking-part slots of largest area (ties: lower slot), then every candidate in slot order, plain before mirrored
    int sel[LOC_MAX_SEEDS];
    const int nsel = loc_top_k(a.max_tags, lane, [&](int k) { return L.area[k]; }, sel);
    auto make = [&](int k) {
        double H[9], To[12], M[12];
        cal_square_h(fo[k].corners, th[2], th[3], s, H);
        double hs = a.half;
        map_tag_half(a.map[fo[k].id], hs);  // the slot's own half
        cal_planar_pose(H, th[0], th[1], s, hs, To);
        const double *Mp = a.map[fo[k].id].T;
#pragma unroll
        for (int i = 0; i < 12; i++) M[i] = Mp[i];
        return [=](bool mirror, double *C) { loc_candidate(To, M, mirror, C, C + 9); };
    };
    double Pb[12], best = INFINITY;
    const int code = loc_best_candidate(sel, nsel, make, [&](const double *C) { return pass(C, C + 9, std::false_type{}, nullptr); }, best, Pb);
    if (!(best < LOC_BEHIND_COST)) {
        if (lane == 0) a.fr[CAL_FR * f] = 3;
        return;
    }
    double *R = Pb, *t = Pb + 9;
    const double cost = pose_lm(pass, R, t);
    double *P = a.pose + (size_t)12 * f;  // buffer 0: cur = 0 at the start
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) P[i] = R[i];
        P[9] = t[0]; P[10] = t[1]; P[11] = t[2];
        a.seedc[f] = cost;
        a.fr[CAL_FR * f + 2] = code;
    }
    cal_linearise<NT>(cam0, (a.flags & CAL_FIX_ASPECT) != 0, a.st->ratio, R, t, L, n4, lane, a.H + (size_t)CAL_HS * f);
}

// ---- the fisheye's seed: one wavefront per (frame, rung)

// f_j = max(width, height) / pi * 2^((j - 4) / 4): the quarter powers of two are four constants times an exact power of two
__device__ __forceinline__ double cal_rung_focal(int j, double width, double height)
{
    const int q = j - 4, m = q & 3, e = (q - m) / 4;  // q = 4 e + m, 0 <= m < 4
    const double quarter = m == 0 ? 1.0 : m == 1 ? 1.189207115002721 : m == 2 ? 1.4142135623730951 : 1.681792830507429;
    const double two_e = e >= 0 ? (double)(1 << e) : 1.0 / (double)(1 << -e);
    return (fmax(width, height) / 3.141592653589793) * (quarter * two_e);
}

__global__ void __launch_bounds__(64) k_calib_fish_seed(CalibArgs a)
{
    extern __shared__ double s_dyn[];
    const int f = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    if (a.st->status != 0 || a.fr[CAL_FR * f] != 0 || j >= a.n_rungs) return;
    const LocLds L = loc_lds(s_dyn, a.max_tags);
    cal_gather(a, f, lane, L);
    const ObsRec *fo = a.obs + (size_t)f * a.max_tags;
    double th[4];
    if (a.has_init) {
#pragma unroll
        for (int i = 0; i < 4; i++) th[i] = a.st->theta[0][i];
    } else {
        th[0] = th[1] = cal_rung_focal(j, a.width, a.height);
        th[2] = 0.5 * a.width; th[3] = 0.5 * a.height;
    }
    const FishDev cam0 = cal_fish(th, 0);
    const CalFishCam model{cam0, a.max_tags};
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return loc_pass<decltype(ne_tag)::value>(model, R, t, L, lane, ne);
    };

    // the gate: a slot with a corner further than CAL_GATE from the axis does not seed (a lane reads back its own slots)
    for (int s = lane; s < a.max_tags; s += ASL_WAVE) {
        if (L.state[s] != 1) continue;
        bool in = true;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double xd = ((double)L.uv[2 * (4 * s + q)] - th[2]) / th[0], yd = ((double)L.uv[2 * (4 * s + q) + 1] - th[3]) / th[1];
            in = in && sqrt(xd * xd + yd * yd) <= CAL_GATE;
        }
        if (!in) L.area[s] = -1.0;
    }
    __syncthreads();
    int sel[LOC_MAX_SEEDS];
    const int nsel = loc_top_k(a.max_tags, lane, [&](int k) { return L.area[k]; }, sel);
    auto make = [&](int k) {
        double c8[8], H[9], To[12], M[12];
#pragma unroll
        for (int q = 0; q < 4; q++) {  // the corner's ray as pinhole coordinates: (tan(theta) / theta) (xd, yd)
            const double xd = ((double)fo[k].corners[2 * q] - th[2]) / th[0], yd = ((double)fo[k].corners[2 * q + 1] - th[3]) / th[1];
            const double ang = sqrt(xd * xd + yd * yd), kk = ang > 0 ? tan(ang) / ang : 1.0;
            c8[2 * q] = kk * xd; c8[2 * q + 1] = kk * yd;
        }
        cal_square_h(c8, 0.0, 0.0, 1.0, H);
        double hs = a.half;
        map_tag_half(a.map[fo[k].id], hs);  // the slot's own half
        cal_planar_pose(H, 1.0, 1.0, 1.0, hs, To);
        const double *Mp = a.map[fo[k].id].T;
#pragma unroll
        for (int i = 0; i < 12; i++) M[i] = Mp[i];
        return [=](bool mirror, double *C) { loc_candidate(To, M, mirror, C, C + 9); };
    };
    double Pb[12], best = INFINITY;
    const int code = loc_best_candidate(sel, nsel, make, [&](const double *C) { return pass(C, C + 9, std::false_type{}, nullptr); }, best, Pb);
    const size_t o = (size_t)f * a.n_rungs + j;
    if (!(best < LOC_BEHIND_COST)) {  // no candidate at this rung: the rung pays LOC_BEHIND_COST for the frame
        if (lane == 0) { a.lcost[o] = LOC_BEHIND_COST; a.lcode[o] = -1; }
        return;
    }
    double *R = Pb, *t = Pb + 9;
    const double cost = pose_lm(pass, R, t);
    if (lane == 0) {
        double *P = a.lpose + 12 * o;
#pragma unroll
        for (int i = 0; i < 9; i++) P[i] = R[i];
        P[9] = t[0]; P[10] = t[1]; P[11] = t[2];
        a.lcost[o] = cost;
        a.lcode[o] = code;
    }
}

// ---- one workgroup: the rungs' scores over the taking-part frames, the winner, theta0, its seeds into place
__global__ void __launch_bounds__(CAL_WG) k_calib_fish_pick(CalibArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64];
    __shared__ int s_any, s_j;
    CalibState *st = a.st;
    if (st->status != 0) return;
    const int n = st->n_take, nr = a.n_rungs;
    cal_list_sum(a.lcost, nr, nr, a.list, n, s_part, s_sum);
    if (threadIdx.x == 0) {
        int jb = 0;
        for (int j = 1; j < nr; j++)
            if (s_sum[j] < s_sum[jb]) jb = j;  // ties: the lower rung
        s_j = jb;
        s_any = 0;
    }
    __syncthreads();
    const int jw = s_j;
    for (int k = threadIdx.x; k < n; k += CAL_WG)
        if (a.lcode[(size_t)a.list[k] * nr + jw] >= 0) s_any = 1;
    __syncthreads();
    // no frame has a candidate at the winning rung: status 2, the frames stay taking part (status 4).  With K_init there is
    // no ladder to fail: the frames are dropped and k_calib_start finds none (status 1), as under the Brown lens.
    const bool none = !s_any && !a.has_init;
    for (int k = threadIdx.x; k < n && !none; k += CAL_WG) {
        const int f = a.list[k];
        const size_t o = (size_t)f * nr + jw;
        if (a.lcode[o] < 0) { a.fr[CAL_FR * f] = 3; continue; }
        for (int i = 0; i < 12; i++) a.pose[(size_t)12 * f + i] = a.lpose[12 * o + i];  // buffer 0: cur = 0 at the start
        a.seedc[f] = a.lcost[o];
        a.fr[CAL_FR * f + 2] = a.lcode[o];
    }
    if (threadIdx.x == 0) {
        if (none) { st->status = 2; st->done = 1; }
        else if (!a.has_init) {
            const double fj = cal_rung_focal(jw, a.width, a.height);
            const double th[4] = {fj, fj, 0.5 * a.width, 0.5 * a.height};
            for (int i = 0; i < 4; i++) { st->theta[0][i] = th[i]; st->theta[1][i] = th[i]; }
        }
    }
}

// ---- per frame: the normal equations at (K0, k = 0, the seed pose)
template <int ND>
__global__ void __launch_bounds__(64) k_calib_fish_lin(CalibArgs a)
{
    constexpr int NT = 11 + ND;
    extern __shared__ double s_dyn[];
    const int f = blockIdx.x, lane = threadIdx.x, n4 = 4 * a.max_tags;
    if (a.st->status != 0 || a.fr[CAL_FR * f] != 0) return;
    const LocLds L = loc_lds(s_dyn, a.max_tags);
    cal_gather(a, f, lane, L);
    const double *P = a.pose + (size_t)12 * f;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = P[i];
    t[0] = P[9]; t[1] = P[10]; t[2] = P[11];
    cal_linearise<NT>(cal_fish(a.st->theta[0], 0), (a.flags & CAL_FIX_ASPECT) != 0, a.st->ratio, R, t, L, n4, lane, a.H + (size_t)CAL_HS * f);
}

// ---- one workgroup: used frames, initial cost, lambda0
__global__ void __launch_bounds__(CAL_WG) k_calib_start(CalibArgs a)
{
    __shared__ int s_cnt[CAL_WG];
    __shared__ double s_part[CAL_WG], s_sum[64];
    CalibState *st = a.st;
    if (st->status != 0) return;
    const int n = cal_make_list(a, s_cnt);
    // corners of the used frames: per-thread partial counts in frame-list order, summed in LDS (integers: exact)
    int c = 0;
    for (int k = threadIdx.x; k < n; k += CAL_WG) c += a.fr[CAL_FR * a.list[k] + 1];
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    cal_list_sum(a.seedc, 1, 1, a.list, n, s_part, s_sum);
    const double seed_cost = s_sum[0];
    const int nt = cal_nt(a.n_dist);
    cal_list_sum(a.H + nt * (nt + 1) / 2 - 1, CAL_HS, 1, a.list, n, s_part, s_sum);
    if (threadIdx.x == 0) {
        int corners = 0;
        for (int i = 0; i < CAL_WG; i++) corners += s_cnt[i];
        corners *= 4;
        st->n_used = n;
        st->n_corners = corners;
        st->seed_cost = seed_cost;
        st->cost = s_sum[0];
        st->lambda = 1e-3;
        if (n == 0 || 2 * (long long)corners <= 6 * (long long)n + a.np) { st->status = 1; st->done = 1; }
    }
}

// ---- per used frame: the pose block eliminated; final = 1: undamped, at the solution (for the uncertainty)
__global__ void __launch_bounds__(64) k_calib_schur(CalibArgs a, int final)
{
    __shared__ double s_H[CAL_HS], s_UW[6 * 9], s_Ug[6];
    const CalibState *st = a.st;
    const int lane = threadIdx.x;
    if (st->status != 0 || (!final && st->done) || (int)blockIdx.x >= st->n_used) return;
    const int f = a.list[blockIdx.x], cur = st->cur, np = a.np, rc = 10 + a.n_dist;  // rc: the residual column
    const double lam1 = final ? 1.0 : 1.0 + st->lambda;
    const double *Hf = a.H + ((size_t)cur * a.n_frames + f) * CAL_HS;
    for (int i = lane; i < CAL_HS; i += ASL_WAVE) s_H[i] = Hf[i];
    __syncthreads();
    double U[21];
#pragma unroll
    for (int i = 0; i < 21; i++) U[i] = s_H[i];
#pragma unroll
    for (int i = 0; i < 6; i++) U[TRI(i, i)] *= lam1;
    // Cholesky of U (every lane, identical), then lane j < np: U^-1 W[:, j]; lane np: U^-1 g_pose
    double b[6] = {0, 0, 0, 0, 0, 0};
    if (lane <= np) {
        const int col = lane < np ? 6 + a.sel[lane] : rc;
#pragma unroll
        for (int i = 0; i < 6; i++) b[i] = s_H[TRI(col, i)];
    }
    const bool ok = chol6_solve_tri_dev(U, b);
    if (lane < np) {
#pragma unroll
        for (int i = 0; i < 6; i++) s_UW[6 * lane + i] = b[i];
    } else if (lane == np) {
#pragma unroll
        for (int i = 0; i < 6; i++) s_Ug[i] = b[i];
    }
    __syncthreads();
    double *SB = a.SB + (size_t)CAL_SB * f, *BK = a.back + (size_t)CAL_BK * f;
    const int ntri = np * (np + 1) / 2;
    if (lane < ntri) {  // S_ij = V_ij - W_i . (U^-1 W)_j
        int i = 0;
        while (TRI(i + 1, 0) <= lane) i++;
        const int j = lane - TRI(i, 0), ci = 6 + a.sel[i], cj = 6 + a.sel[j];
        double v = s_H[TRI(ci, cj)];
        if (i == j) v *= lam1;
        for (int k = 0; k < 6; k++) v -= s_H[TRI(ci, k)] * s_UW[6 * j + k];
        SB[lane] = v;
    } else if (lane >= CAL_SB_B && lane < CAL_SB_B + np) {  // b_i = g_i - W_i . U^-1 g_pose
        const int i = lane - CAL_SB_B, ci = 6 + a.sel[i];
        double v = s_H[TRI(rc, ci)];
        for (int k = 0; k < 6; k++) v -= s_H[TRI(ci, k)] * s_Ug[k];
        SB[lane] = v;
    }
    if (lane < 6 * np) BK[lane] = s_UW[lane];
    else if (lane >= 54 && lane < 60) BK[lane] = s_Ug[lane - 54];
    if (lane == 0) a.fr[CAL_FR * f + 3] = ok ? 1 : 0;
}

// ---- one workgroup: the reduced system, d_theta, the trial theta
__global__ void __launch_bounds__(CAL_WG) k_calib_solve(CalibArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64];
    __shared__ int s_bad;
    CalibState *st = a.st;
    if (st->status != 0 || st->done) return;
    const int n = st->n_used, np = a.np;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += CAL_WG)
        if (a.fr[CAL_FR * a.list[k] + 3] == 0) s_bad = 1;
    cal_list_sum(a.SB, CAL_SB, 64, a.list, n, s_part, s_sum);
    if (threadIdx.x == 0) {
        double *d = s_part;  // LDS: the free entries are indexed at run time
        for (int i = 0; i < np; i++) d[i] = -s_sum[CAL_SB_B + i];
        const bool ok = !s_bad && cal_chol(s_sum, d, np);
        st->solve_ok = ok;
        if (ok) {  // the trial theta: fixed entries keep their bits, fx = r fy under a fixed aspect ratio
            const int cur = st->cur;
            double *tn = st->theta[1 - cur];
            for (int i = 0; i < 9; i++) { tn[i] = st->theta[cur][i]; st->dtheta[i] = i < np ? d[i] : 0.0; }
            for (int j = 0; j < np; j++) tn[a.sel[j]] = st->theta[cur][a.sel[j]] + d[j];
            if (a.flags & CAL_FIX_ASPECT) tn[0] = st->ratio * tn[1];
        }
    }
}

// ---- per used frame: the pose step, the trial pose and its normal equations
template <int ND, int LENS = CAL_LENS_BROWN>
__global__ void __launch_bounds__(64) k_calib_step(CalibArgs a)
{
    constexpr int NT = 11 + ND;
    extern __shared__ double s_dyn[];
    const CalibState *st = a.st;
    const int lane = threadIdx.x, n4 = 4 * a.max_tags;
    if (st->status != 0 || st->done || !st->solve_ok || (int)blockIdx.x >= st->n_used) return;
    const int f = a.list[blockIdx.x], cur = st->cur, np = a.np;
    const double *BK = a.back + (size_t)CAL_BK * f, *P = a.pose + ((size_t)cur * a.n_frames + f) * 12;
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = 0;
        for (int j = 0; j < np; j++) v += BK[6 * j + i] * st->dtheta[j];
        d[i] = -(BK[54 + i] + v);
    }
    double R0[9], t0[3], dR[9], R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R0[i] = P[i];
    t0[0] = P[9]; t0[1] = P[10]; t0[2] = P[11];
    rodrigues_dev(d, dR);
    mat3_mul_dev(dR, R0, R);
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = dR[3 * r] * t0[0] + dR[3 * r + 1] * t0[1] + dR[3 * r + 2] * t0[2] + d[3 + r];
    double *Pn = a.pose + ((size_t)(1 - cur) * a.n_frames + f) * 12;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) Pn[i] = R[i];
        Pn[9] = t[0]; Pn[10] = t[1]; Pn[11] = t[2];
    }
    const LocLds L = loc_lds(s_dyn, a.max_tags);
    cal_gather(a, f, lane, L);
    double *Hn = a.H + ((size_t)(1 - cur) * a.n_frames + f) * CAL_HS;
    if constexpr (LENS == CAL_LENS_FISHEYE)
        cal_linearise<NT>(cal_fish(st->theta[1 - cur], ND), (a.flags & CAL_FIX_ASPECT) != 0, st->ratio, R, t, L, n4, lane, Hn);
    else
        cal_linearise<NT>(cal_cam(st->theta[1 - cur], ND, a.half), (a.flags & CAL_FIX_ASPECT) != 0, st->ratio, R, t, L, n4, lane, Hn);
}

// ---- one workgroup: accept or reject the trial
__global__ void __launch_bounds__(CAL_WG) k_calib_decide(CalibArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64];
    CalibState *st = a.st;
    if (st->status != 0 || st->done) return;
    const int cur = st->cur, nt = cal_nt(a.n_dist);
    const bool solved = st->solve_ok;
    if (solved) cal_list_sum(a.H + ((size_t)(1 - cur) * a.n_frames) * CAL_HS + nt * (nt + 1) / 2 - 1, CAL_HS, 1, a.list, st->n_used, s_part, s_sum);
    if (threadIdx.x == 0) {
        st->iterations += 1;
        const double cost = st->cost;
        if (solved && s_sum[0] < cost) {
            const double cn = s_sum[0];
            st->cost = cn;
            st->cur = 1 - cur;
            st->lambda *= 0.1;
            if (cost - cn < 1e-12 * cost) st->done = 1;
        } else
            st->lambda *= 10;
        if (st->iterations >= a.max_iters) st->done = 1;
    }
}

// ---- one workgroup: the uncertainty from the undamped reduced system, the result and the per-frame records
__global__ void __launch_bounds__(CAL_WG) k_calib_finish(CalibArgs a)
{
    __shared__ double s_part[CAL_WG], s_sum[64], s_x[9 * 9], s_sd[9];
    __shared__ int s_bad;
    CalibState *st = a.st;
    const int np = a.np, cur = st->cur;
    int status = st->status;
    const double *th = st->theta[cur];
    if (status == 0) {
        bool fin = isfinite(st->cost);
        for (int i = 0; i < 9; i++) fin = fin && isfinite(th[i]);
        if (!fin) status = 3;
    }
    if (threadIdx.x < 9) s_sd[threadIdx.x] = 0;
    __syncthreads();
    if (status == 0) {
        cal_list_sum(a.SB, CAL_SB, 64, a.list, st->n_used, s_part, s_sum);
        if (threadIdx.x == 0) s_bad = !cal_chol(s_sum, nullptr, np);
        __syncthreads();
        if ((int)threadIdx.x < np) {  // column i of S^-1 from the factor in s_sum; std of the free entry i
            double *x = s_x + 9 * threadIdx.x;
            const int i = threadIdx.x;
            for (int k = 0; k < np; k++) x[k] = k == i ? 1.0 : 0.0;
            for (int r = 0; r < np; r++) {
                double v = x[r];
                for (int k = 0; k < r; k++) v -= s_sum[TRI(r, k)] * x[k];
                x[r] = v / s_sum[TRI(r, r)];
            }
            for (int r = np - 1; r >= 0; r--) {
                double v = x[r];
                for (int k = r + 1; k < np; k++) v -= s_sum[TRI(k, r)] * x[k];
                x[r] = v / s_sum[TRI(r, r)];
            }
            const double sigma2 = st->cost / (double)(2 * st->n_corners - 6 * st->n_used - np);
            s_sd[a.sel[i]] = s_bad ? NAN : sqrt(sigma2 * x[i]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        CalibResultRec *r = a.res;
        for (int i = 0; i < 9; i++) r->K[i] = 0;
        for (int i = 0; i < 5; i++) r->dist[i] = 0;
        for (int i = 0; i < 9; i++) r->std[i] = s_sd[i];
        r->rms_px = 0; r->rms_init_px = 0;
        if (status == 0) {
            r->K[0] = th[0]; r->K[2] = th[2]; r->K[4] = th[1]; r->K[5] = th[3]; r->K[8] = 1.0;
            for (int i = 0; i < a.n_dist; i++) r->dist[i] = th[4 + i];
            r->rms_px = sqrt(st->cost / st->n_corners);
        }
        if (status == 0 || status == 3) r->rms_init_px = sqrt(st->seed_cost / st->n_corners);  // the seed ran
        r->n_frames_used = st->n_used; r->n_corners = st->n_corners; r->iterations = st->iterations; r->status = status;
    }
    const int nt = cal_nt(a.n_dist);
    for (int f = threadIdx.x; f < a.n_frames; f += CAL_WG) {
        const int *fr = a.fr + CAL_FR * f;
        CamPoseRec *o = a.out + f;
        for (int i = 0; i < 16; i++) o->T[i] = (i % 5 == 0) ? 1.0 : 0.0;
        o->rms_px = 0; o->n_tags = fr[1]; o->n_rejected = 0; o->seed_slot = fr[2];
        o->rms_seed_px = fr[2] >= 0 ? sqrt(a.seedc[f] / (4.0 * fr[1])) : 0.0;
        if (fr[0] != 0) { o->status = fr[0]; continue; }
        if (status != 0) { o->status = 4; continue; }
        const double *P = a.pose + ((size_t)cur * a.n_frames + f) * 12, *R = P, *t = P + 9;
        for (int r = 0; r < 3; r++) {
            o->T[4 * r] = R[r]; o->T[4 * r + 1] = R[3 + r]; o->T[4 * r + 2] = R[6 + r];
            o->T[4 * r + 3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
        }
        o->rms_px = sqrt(a.H[((size_t)cur * a.n_frames + f) * CAL_HS + nt * (nt + 1) / 2 - 1] / (4.0 * fr[1]));
        o->status = 0;
    }
}
