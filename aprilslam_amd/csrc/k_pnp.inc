// S9: batched planar PnP, a quad of lanes per tag, float64 throughout.
// Replaces cv2.solvePnP(obj, corners, K, dist) [ITERATIVE] + cv2.Rodrigues per detection
// (reference tag_detector.py:30-52): undistort -> exact 4-point homography -> pose from the
// homography (nearest rotation) -> Levenberg-Marquardt on the 8 pixel residuals.
// Tags are independent and tiny (8 residuals x 6 dof): latency-bound scalar math, so the
// parallel axis is the tag, not the matrix; MFMA has nothing to contribute here.

__device__ __forceinline__ void mat3_mul_dev(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ void rodrigues_dev(const double r[3], double R[9])
{
    double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < 2.220446049250313e-16) {
        R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
        return;
    }
    double c, s;
    sincos(theta, &s, &c);  // one argument reduction for both
    const double c1 = 1 - c, it = 1 / theta;
    double x = r[0] * it, y = r[1] * it, z = r[2] * it;
    R[0] = c + c1 * x * x;     R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
    R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y;     R[5] = c1 * y * z - s * x;
    R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
}

__device__ __forceinline__ void rot_to_rvec_dev(const double *R, double r[3])
{
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1 ? 1 : (c < -1 ? -1 : c);
    double theta = atan2(s, c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = 0; r[1] = 0; r[2] = 0; return; }
        double t;
        t = (R[0] + 1) * 0.5; rx = sqrt(t > 0 ? t : 0);
        t = (R[4] + 1) * 0.5; ry = sqrt(t > 0 ? t : 0) * (R[1] < 0 ? -1.0 : 1.0);
        t = (R[8] + 1) * 0.5; rz = sqrt(t > 0 ? t : 0) * (R[2] < 0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
        theta /= sqrt(rx * rx + ry * ry + rz * rz);
        r[0] = theta * rx; r[1] = theta * ry; r[2] = theta * rz;
        return;
    }
    double vth = 1 / (2 * s) * theta;
    r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
}

__device__ __forceinline__ void jacobi3_dev(double A[9], double V[9], double d[3])
{
    for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = fabs(A[1]) + fabs(A[2]) + fabs(A[5]);
        // relative stop: below this the remaining rotations are identity in float64
        if (off < 1e-15 * (fabs(A[0]) + fabs(A[4]) + fabs(A[8]))) break;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                double apq = A[3 * p + q];
                if (fabs(apq) < 1e-300) continue;
                double theta = (A[3 * q + q] - A[3 * p + p]) / (2 * apq);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double akp = A[3 * k + p], akq = A[3 * k + q];
                    A[3 * k + p] = c * akp - s * akq;
                    A[3 * k + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double apk = A[3 * p + k], aqk = A[3 * q + k];
                    A[3 * p + k] = c * apk - s * aqk;
                    A[3 * q + k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double vkp = V[3 * k + p], vkq = V[3 * k + q];
                    V[3 * k + p] = c * vkp - s * vkq;
                    V[3 * k + q] = s * vkp + c * vkq;
                }
            }
    }
    d[0] = A[0]; d[1] = A[4]; d[2] = A[8];
}

__device__ __forceinline__ void nearest_rotation_dev(const double *M, double *R)
{
    double S[9], V[9], d[3], Mt[9], W[9], T[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Mt[3 * i + j] = M[3 * j + i];
    mat3_mul_dev(Mt, M, S);
    jacobi3_dev(S, V, d);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += V[3 * i + k] * (1 / sqrt(d[k] > 1e-300 ? d[k] : 1e-300)) * V[3 * j + k];
            W[3 * i + j] = acc;
        }
    mat3_mul_dev(M, W, T);
    for (int i = 0; i < 9; i++) R[i] = T[i];
}

__device__ __forceinline__ void undistort_dev(const CamDev &c, double u, double v, double *xo, double *yo)
{
    double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy, x = x0, y = y0;
    if (c.k1 != 0 || c.k2 != 0 || c.p1 != 0 || c.p2 != 0 || c.k3 != 0)
        for (int it = 0; it < 5; it++) {
            double r2 = x * x + y * y;
            double icdist = 1 / (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
            double dx = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
            double dy = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
    *xo = x; *yo = y;
}

__device__ __forceinline__ void project_dev(const CamDev &c, const double P[3], double uv[2], double *J)
{
    double iz = 1 / P[2], x = P[0] * iz, y = P[1] * iz;
    double r2 = x * x + y * y;
    double cd = 1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    double dcd = c.k1 + r2 * (2 * c.k2 + 3 * c.k3 * r2);
    double xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
    double yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
    uv[0] = c.fx * xd + c.cx;
    uv[1] = c.fy * yd + c.cy;
    if (!J) return;
    double dxd_dx = cd + x * dcd * 2 * x + 2 * c.p1 * y + c.p2 * (2 * x + 4 * x);
    double dxd_dy = x * dcd * 2 * y + 2 * c.p1 * x + c.p2 * 2 * y;
    double dyd_dx = y * dcd * 2 * x + c.p1 * 2 * x + 2 * c.p2 * y;
    double dyd_dy = cd + y * dcd * 2 * y + c.p1 * (2 * y + 4 * y) + 2 * c.p2 * x;
    double dx_dP[3] = {iz, 0, -x * iz}, dy_dP[3] = {0, iz, -y * iz};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        J[k] = c.fx * (dxd_dx * dx_dP[k] + dxd_dy * dy_dP[k]);
        J[3 + k] = c.fy * (dyd_dx * dx_dP[k] + dyd_dy * dy_dP[k]);
    }
}

// ---- One tag is solved by a QUAD of lanes, lane q of the quad = corner q.  Everything per corner (undistortion,
// projection, its two rows of the Jacobian and their contribution to the normal equations) is done by the corner's lane;
// the four contributions are added by butterfly_sum<4> (k_wave.inc: the same bits in all four lanes), and the small serial
// parts (6x6 Cholesky, Rodrigues, the 3x3 Jacobi sweep) are computed redundantly by the four lanes on identical inputs --
// their control flow is identical too.  Against one thread per tag this halves the serial chain of a Levenberg-Marquardt
// trial, fills every lane of a wave with 16 tags instead of 64 (a wave runs as long as its slowest tag: the trip count has
// a heavy tail), and the normal equations keep only their lower triangle: the kernel fits 128 registers without scratch
// (one thread per tag: 256 + 56 and 304 bytes of scratch).

// index of (a, b), a >= b, in the packed lower triangle
#define TRI(a, b) ((a) * ((a) + 1) / 2 + (b))

// 6x6 SPD solve from the packed lower triangle A (21 entries, overwritten by its Cholesky factor), b overwritten with x.
// One reciprocal per pivot; every other division of the factorisation and of the two triangular solves becomes a
// multiplication (float64 division is a ~40-instruction sequence and this chain is serial).
__device__ __forceinline__ bool chol6_solve_tri_dev(double *A, double *b)
{
    double inv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = A[TRI(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[TRI(i, k)] * A[TRI(j, k)];
            if (i == j) {
                if (!(s > 0)) return false;
                A[TRI(i, i)] = sqrt(s);
                inv[i] = 1 / A[TRI(i, i)];
            } else
                A[TRI(i, j)] = s * inv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= A[TRI(i, k)] * b[k];
        b[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= A[TRI(k, i)] * b[k];
        b[i] = s * inv[i];
    }
    return true;
}

// ---- first-order pose covariance (asl_pose_cov), shared by k_localize<true> (k_localize.inc) and k_pnp_cov (k_posecov.inc)

struct PoseCovRec {  // == asl_pose_cov, 304 bytes
    double cov[36];
    double sigma_px;
    int32_t dof, status;
};

// A pivot of the undamped Cholesky below this fraction of its diagonal entry means the normal matrix has no positive
// definite meaning left in float64 (Jacobi-scaled condition number past ~1e13): status 2 (tests/pose_cov_ref.py: PIVOT_TOL)
#define POSE_COV_PIVOT_TOL 1e-13

// Column c (0..5) of (J^T J)^-1 in the output convention of asl_pose_cov.  H: the packed lower triangle of J^T J in the
// solvers' own coordinates (w, v) of the left update R <- Rod(w) R, t <- Rod(w) t + v on camera<-X = (R, t).  The
// output error (r, d) = A (w, v) to first order, so column c of A H^-1 A^T is A x with H x = A^T e_c: one Cholesky
// (the same in every lane that holds the same H) and one pair of triangular solves per column, and no lane ever holds
// the whole inverse.
//   WFC (world<-camera = inverse of (R, t)):  A = diag(-R^T, -R^T)
//   else (camera<-tag = (R, t) itself):       A = [I 0; -[t]x I]
// false: H is not positive definite (col is not written).
template <bool WFC>
__device__ __forceinline__ bool pose_cov_column_dev(const double *H, const double *R, const double *t, int c, double *col)
{
    // c picks by a one-hot product, not by an index or a chain of selects: either makes the compiler keep R in scratch
    const int k = c < 3 ? c : c - 3;
    const double e0 = k == 0 ? 1.0 : 0.0, e1 = k == 1 ? 1.0 : 0.0, e2 = k == 2 ? 1.0 : 0.0, lo = c < 3 ? 1.0 : 0.0, hi = 1.0 - lo;
    double A[21], x[6];
#pragma unroll
    for (int i = 0; i < 21; i++) A[i] = H[i];
    if constexpr (WFC) {  // A^T e_c: column k of -R in the block of c
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double m = -(R[3 * i] * e0 + R[3 * i + 1] * e1 + R[3 * i + 2] * e2);
            x[i] = lo * m;
            x[3 + i] = hi * m;
        }
    } else {  // A^T = [I [t]x; 0 I]: e_k, or column k of [t]x over e_k
        x[0] = lo * e0 + hi * (t[1] * e2 - t[2] * e1);
        x[1] = lo * e1 + hi * (t[2] * e0 - t[0] * e2);
        x[2] = lo * e2 + hi * (t[0] * e1 - t[1] * e0);
        x[3] = hi * e0; x[4] = hi * e1; x[5] = hi * e2;
    }
    if (!chol6_solve_tri_dev(A, x)) return false;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (!(A[TRI(i, i)] * A[TRI(i, i)] > POSE_COV_PIVOT_TOL * H[TRI(i, i)])) return false;
    if constexpr (WFC) {
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 3; i++) col[3 * b + i] = -(R[i] * x[3 * b] + R[3 + i] * x[3 * b + 1] + R[6 + i] * x[3 * b + 2]);
    } else {
        col[0] = x[0]; col[1] = x[1]; col[2] = x[2];
        col[3] = x[3] - (t[1] * x[2] - t[2] * x[1]);
        col[4] = x[4] - (t[2] * x[0] - t[0] * x[2]);
        col[5] = x[5] - (t[0] * x[1] - t[1] * x[0]);
    }
    return true;
}

// sigma^2 and the record's sigma_px / dof: the given sigma, or cost / dof of the solve for sigma_px == 0
__device__ __forceinline__ double pose_cov_sigma2(double sigma_px, double cost, int dof, double *sigma_out)
{
    const double s2 = sigma_px > 0 ? sigma_px * sigma_px : cost / (double)dof;
    *sigma_out = sigma_px > 0 ? sigma_px : sqrt(s2);
    return s2;
}

// Column c of the scaled covariance into the record, by the lane that solved it: its entries on and below the diagonal
// go to both triangles, so the stored matrix is symmetric to the bit.  ok false: zeros.
__device__ __forceinline__ void pose_cov_store_column(PoseCovRec *o, int c, const double *col, double s2, bool ok)
{
#pragma unroll
    for (int r = 0; r < 6; r++) {
        if (r < c) continue;
        const double v = ok ? s2 * col[r] : 0.0;
        o->cov[6 * r + c] = v;
        o->cov[6 * c + r] = v;
    }
}

#define PNP_TAGS_PER_WAVE 16
#define PNP_NE 27  /* the normal equations of a tag: 21 entries of JtJ (packed lower triangle) + 6 of Jt r */

// A tag's normal equations live in LDS between the linearisation and the (possibly repeated) damped solves: entry k of
// quad gi at ne[k * 16], ne = base + gi.  Written by the four lanes alike (same value, same address), read by all four (a
// broadcast); the four lanes run the same control path and a wave's LDS operations execute in program order, so no barrier is needed.
__device__ __forceinline__ void pnp_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// This lane's corner: squared pixel residual, and optionally its part of JtJ (packed lower triangle) and Jt r -- summed over
// the quad and parked in `ne`.  Corner (ox, oy, 0) of the tag, image point (iu, iv).
__device__ __forceinline__ double pnp_accumulate_quad(const CamDev &c, const double *R, const double *t, double ox, double oy, double iu, double iv,
                                                      double *ne, int q)
{
    double RX[3], P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        RX[r] = R[3 * r] * ox + R[3 * r + 1] * oy;
        P[r] = RX[r] + t[r];
    }
    project_dev(c, P, uv, ne ? Jp : nullptr);
    const double r0 = uv[0] - iu, r1 = uv[1] - iv;
    const double cost = butterfly_sum<4>(r0 * r0 + r1 * r1);
    if (ne) {
        // P(dw) = exp([dw]x) R X + t  ->  dP/dw = -[RX]x ,  dP/dt = I
        const double dPdw[9] = {0, RX[2], -RX[1], -RX[2], 0, RX[0], RX[1], -RX[0], 0};
        double J0[6], J1[6];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            J0[k] = Jp[0] * dPdw[k] + Jp[1] * dPdw[3 + k] + Jp[2] * dPdw[6 + k];
            J0[3 + k] = Jp[k];
            J1[k] = Jp[3] * dPdw[k] + Jp[4] * dPdw[3 + k] + Jp[5] * dPdw[6 + k];
            J1[3 + k] = Jp[3 + k];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double ga = butterfly_sum<4>(J0[a] * r0 + J1[a] * r1);
            ne[(21 + a) * PNP_TAGS_PER_WAVE] = ga;  // all four lanes: the same value to the same address (no branch, the sum's register is free at once)
#pragma unroll
            for (int b = 0; b <= a; b++) {
                const double hab = butterfly_sum<4>(J0[a] * J0[b] + J1[a] * J1[b]);
                ne[TRI(a, b) * PNP_TAGS_PER_WAVE] = hab;
            }
        }
        pnp_lds_order();
    }
    return cost;
}

// Levenberg-Marquardt on the 8 pixel residuals from (R, t), run by the four lanes of a quad in lockstep; returns the final cost
__device__ double pnp_lm_quad(const CamDev &c, double *R, double *t, double ox, double oy, double iu, double iv, double *ne, int q)
{
    double cost = pnp_accumulate_quad(c, R, t, ox, oy, iu, iv, ne, q);
    double lambda = 1e-3;
    for (int it = 0; it < 20; it++) {  // OpenCV caps its LM at 20 iterations as well
        bool improved = false;
        double step_norm = 0;
        for (int tries = 0; tries < 12 && !improved; tries++) {
            double Aa[21], d[6];
#pragma unroll
            for (int i = 0; i < 21; i++) Aa[i] = ne[i * PNP_TAGS_PER_WAVE];
#pragma unroll
            for (int a = 0; a < 6; a++) { Aa[TRI(a, a)] += lambda * (Aa[TRI(a, a)] > 1e-12 ? Aa[TRI(a, a)] : 1e-12); d[a] = -ne[(21 + a) * PNP_TAGS_PER_WAVE]; }
            if (!chol6_solve_tri_dev(Aa, d)) { lambda *= 10; continue; }
            double dR[9], Rn[9], tn[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
            rodrigues_dev(d, dR);
            mat3_mul_dev(dR, R, Rn);
            const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
            const double costn = pnp_accumulate_quad(c, Rn, tn, ox, oy, iu, iv, nullptr, q);
            if (costn < cost) {
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
                t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
                step_norm = dn;
                improved = true;
                lambda *= 0.1;
                if (lambda < 1e-12) lambda = 1e-12;
            } else {
                // a rejected step this small means the minimum is reached: more damping cannot help
                if (dn < 1e-10 * (sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + 1)) break;
                lambda *= 10;
            }
        }
        if (!improved) break;
        const double prev = cost;
        cost = pnp_accumulate_quad(c, R, t, ox, oy, iu, iv, ne, q);
        const double scale = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) + 1;
        if (step_norm < 1e-10 * scale || prev - cost < 1e-15 * (1 + prev)) break;
    }
    return cost;
}

// (iu, iv): this lane's corner of the tag (corner q = lane & 3 of lb, rb, rt, lt = (-h,-h) (h,-h) (h,h) (-h,h)); all lanes of the
// wave must call it (lanes of a quad without a tag compute on a dummy square).  rvec / tvec / T are the same in the four lanes.
__device__ bool pnp_quad_dev(double iu, double iv, int q, const CamDev &c, double *ne, double *rvec, double *tvec, double *T)
{
    // 1-2: exact 4-point homography plane -> normalised image, closed form for a square; every lane undistorts its own corner
    double xq, yq;
    undistort_dev(c, iu, iv, &xq, &yq);
    const double xs[4] = {quad_bcast<0>(xq), quad_bcast<1>(xq), quad_bcast<2>(xq), quad_bcast<3>(xq)};
    const double ys[4] = {quad_bcast<0>(yq), quad_bcast<1>(yq), quad_bcast<2>(yq), quad_bcast<3>(yq)};
    double dx1 = xs[1] - xs[2], dx2 = xs[3] - xs[2], sx = xs[0] - xs[1] + xs[2] - xs[3];
    double dy1 = ys[1] - ys[2], dy2 = ys[3] - ys[2], sy = ys[0] - ys[1] + ys[2] - ys[3];
    double den = dx1 * dy2 - dy1 * dx2;
    if (!(fabs(den) > 1e-300)) return false;
    double gg = (sx * dy2 - sy * dx2) / den, hh = (dx1 * sy - dy1 * sx) / den;
    // unit-square map (u,v) -> image, then (X,Y) -> (u,v) = (X/(2h) + 1/2, Y/(2h) + 1/2)
    double Hs[9] = {xs[1] - xs[0] + gg * xs[1], xs[3] - xs[0] + hh * xs[3], xs[0],
                    ys[1] - ys[0] + gg * ys[1], ys[3] - ys[0] + hh * ys[3], ys[0], gg, hh, 1.0};
    double inv2h = 1 / (2 * c.half), H[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        H[3 * r] = Hs[3 * r] * inv2h;
        H[3 * r + 1] = Hs[3 * r + 1] * inv2h;
        H[3 * r + 2] = 0.5 * Hs[3 * r] + 0.5 * Hs[3 * r + 1] + Hs[3 * r + 2];
    }
    if (!(fabs(H[8]) > 1e-300)) return false;
    double ih = 1 / H[8];  // h33 = 1, and with it t_z > 0 for a tag in front of the camera
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] *= ih;

    // 3: pose from the homography
    const double EPS = 2.220446049250313e-16;
    double h1n = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]);
    double h2n = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
    double i1 = 1 / (h1n > EPS ? h1n : EPS), i2 = 1 / (h2n > EPS ? h2n : EPS);
    double ts = 2 / ((h1n + h2n) > EPS ? (h1n + h2n) : EPS);
    double M[9], R[9], t[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { M[3 * r] = H[3 * r] * i1; M[3 * r + 1] = H[3 * r + 1] * i2; t[r] = H[3 * r + 2] * ts; }
    M[2] = M[3] * M[7] - M[6] * M[4];
    M[5] = M[6] * M[1] - M[0] * M[7];
    M[8] = M[0] * M[4] - M[3] * M[1];
    nearest_rotation_dev(M, R);

    // 4: Levenberg-Marquardt on the 8 pixel residuals
    const double ox = (q == 1 || q == 2) ? c.half : -c.half, oy = (q >= 2) ? c.half : -c.half;
    double cost = pnp_lm_quad(c, R, t, ox, oy, iu, iv, ne, q);
    if (c.both_minima) {
        // A planar target has a second pose that reprojects almost as well (the tag tilted the other way about the viewing
        // ray); cv2.solvePnP(ITERATIVE) -- and so the default here -- returns whichever minimum the homography start falls
        // into.  With the option on, the mirrored start is refined too and the lower reprojection error wins (what IPPE's
        // two-solution test does).  Mirror: tag normal n = R[:,2] reflected about the ray v through the tag centre.
        const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        if (tn > 0) {
            const double v[3] = {t[0] / tn, t[1] / tn, t[2] / tn}, n[3] = {R[2], R[5], R[8]};
            const double nv = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
            const double m[3] = {2 * nv * v[0] - n[0], 2 * nv * v[1] - n[1], 2 * nv * v[2] - n[2]};
            double ax[3] = {n[1] * m[2] - n[2] * m[1], n[2] * m[0] - n[0] * m[2], n[0] * m[1] - n[1] * m[0]};
            const double sn = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), cs = n[0] * m[0] + n[1] * m[1] + n[2] * m[2];
            if (sn > 1e-6) {  // a frontal tag has no second pose
                const double ang = atan2(sn, cs);
                const double w[3] = {ax[0] / sn * ang, ax[1] / sn * ang, ax[2] / sn * ang};
                double Q[9], R2[9], t2[3] = {t[0], t[1], t[2]};
                rodrigues_dev(w, Q);
                mat3_mul_dev(Q, R, R2);
                const double cost2 = pnp_lm_quad(c, R2, t2, ox, oy, iu, iv, ne, q);
                if (cost2 < cost) {
#pragma unroll
                    for (int i = 0; i < 9; i++) R[i] = R2[i];
                    t[0] = t2[0]; t[1] = t2[1]; t[2] = t2[2];
                    cost = cost2;
                }
            }
        }
    }
    nearest_rotation_dev(R, R);
    rot_to_rvec_dev(R, rvec);
    tvec[0] = t[0]; tvec[1] = t[1]; tvec[2] = t[2];
    double Rr[9];
    rodrigues_dev(rvec, Rr);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        T[4 * r] = Rr[3 * r]; T[4 * r + 1] = Rr[3 * r + 1]; T[4 * r + 2] = Rr[3 * r + 2]; T[4 * r + 3] = t[r];
    }
    T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    for (int k = 0; k < 3; k++) if (!isfinite(rvec[k]) || !isfinite(tvec[k])) return false;
    return true;
}

// poses for the detections appended by k_decode (corners rounded to float32 first, as
// np.array(detection['lb-rb-rt-lt'], dtype=np.float32) does in tag_detector.py:32); a quad of lanes per tag, `tpw` tags
// per wave (the LM trip count has a heavy tail -- median 5 tries, 99th percentile 14 -- and a wave runs as long as its
// slowest tag, so a launch that cannot fill the chip anyway spreads its tags over more waves)
__global__ void __launch_bounds__(64) k_pnp_dets(DetRec *dets, const long long *counters, unsigned int max_dets, CamDev cam, int tpw)
{
    __shared__ double s_ne[PNP_NE * PNP_TAGS_PER_WAVE];
    const int lane = threadIdx.x, gi = lane >> 2, q = lane & 3;
    if (batch_poisoned(counters)) return;
    long long n64 = counters[CNT_NDETS];
    unsigned int n = n64 > (long long)max_dets ? max_dets : (unsigned int)n64;
    if (blockIdx.x * (unsigned int)tpw >= n) return;  // no tag in this wave
    const unsigned int i = blockIdx.x * (unsigned int)tpw + (unsigned int)gi;
    const bool have = gi < tpw && i < n;  // the DPP exchanges need every lane of the wave: idle quads solve a dummy square
    const double iu = have ? (double)(float)dets[i].corners[q][0] : ((q == 1 || q == 2) ? 1.0 : -1.0) + cam.cx;
    const double iv = have ? (double)(float)dets[i].corners[q][1] : ((q >= 2) ? 1.0 : -1.0) + cam.cy;
    double rvec[3], tvec[3], T[16];
    const bool ok = pnp_quad_dev(iu, iv, q, cam, s_ne + gi, rvec, tvec, T);
    if (!have) return;
    // the four lanes hold the same result: each writes a quarter of it
    // a tag without a pose (ok false) stores zeros: pnp_quad_dev may have returned before it wrote rvec, tvec or T
    if (q < 3) { dets[i].rvec[q] = ok ? rvec[q] : 0.0; dets[i].tvec[q] = ok ? tvec[q] : 0.0; }
    else dets[i].pose_ok = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) dets[i].T[4 * q + k] = ok ? (q == 0 ? T[k] : (q == 1 ? T[4 + k] : (q == 2 ? T[8 + k] : T[12 + k]))) : 0.0;
}

__global__ void __launch_bounds__(64) k_pnp_batch(const float *corners, int n, CamDev cam, double *rvec, double *tvec, double *T, uint8_t *ok, int tpw)
{
    __shared__ double s_ne[PNP_NE * PNP_TAGS_PER_WAVE];
    const int lane = threadIdx.x, gi = lane >> 2, q = lane & 3;
    const int i = blockIdx.x * tpw + gi;
    const bool have = gi < tpw && i < n;
    const double iu = have ? (double)corners[8 * i + 2 * q] : ((q == 1 || q == 2) ? 1.0 : -1.0) + cam.cx;
    const double iv = have ? (double)corners[8 * i + 2 * q + 1] : ((q >= 2) ? 1.0 : -1.0) + cam.cy;
    double r[3], t[3], TT[16];
    const bool good = pnp_quad_dev(iu, iv, q, cam, s_ne + gi, r, t, TT);
    if (!have) return;
    if (q < 3) { rvec[3 * i + q] = good ? r[q] : 0.0; tvec[3 * i + q] = good ? t[q] : 0.0; }  // no pose: zeros, as in k_pnp_dets
    else ok[i] = good ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 4; k++) T[16 * i + 4 * q + k] = good ? (q == 0 ? TT[k] : (q == 1 ? TT[4 + k] : (q == 2 ? TT[8 + k] : TT[12 + k]))) : 0.0;
}
