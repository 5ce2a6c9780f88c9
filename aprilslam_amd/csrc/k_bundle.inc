// Tag bundles: the pose of one bundle in another's frame, with its covariance (asl_bundle_relative_device /
// asl_bundle_relative_batch).  The poses come from the bundle dimension of k_localize / k_localize_rig (loc_bundle_map,
// k_localize.inc): record f * n_bundles + b holds T_b = bundle_b<-camera (bundle_b<-rig) of frame f and, if asked for, its
// covariance in the (r, d) convention of asl_pose_cov (R_true = Rod(r) R, p_true = p + d).
// One lane per (frame, bundle), float64, no atomics, every sum in a fixed order: the same input gives the same bytes.
// With a = ref, T_a = [R_a | p_a], T_b = [R_b | p_b]:
//   R_ab = R_a R_b^T,  q = R_ab p_b,  p_ab = p_a - q                      T_ab = ref<-bundle_b = T_a inv(T_b)
//   r_ab = r_a - R_ab r_b,  d_ab = d_a + [q]x r_ab - R_ab d_b             to first order
//   J_a = [I 0; [q]x I],  J_b = [-R_ab 0; -[q]x R_ab  -R_ab] = -J_a diag(R_ab, R_ab)
//   C_ab = J_a C_a J_a^T + J_b C_b J_b^T = J_a (C_a + D C_b D^T) J_a^T,   D = diag(R_ab, R_ab)
// The sum takes the two solves as independent: they share no corner (no tag id is valid in two bundles) and the camera
// model they share is exact.  tests/bundle_ref.py is the NumPy statement; its Jacobians are checked against central
// differences of the exact composition (tests/test_bundle_ref.py).
// Latency-bound scalar float64: 464 bytes in per pose pair, 424 out; a frame's lanes read the reference's record together.

struct BundleRelRec {  // == asl_bundle_rel, 424 bytes
    double T[16];
    double cov[36];
    int32_t status, reserved;
};

// S = sym(A M A^T) for 6 x 6 row-major A and M (M symmetric): the lower triangle computed, both triangles written from it
__device__ __forceinline__ void bundle_congruence(const double *A, const double *M, double *S)
{
    double U[36];  // A M
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += A[6 * i + k] * M[6 * k + j];
            U[6 * i + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += U[6 * i + k] * A[6 * j + k];
            S[6 * i + j] = s;
            S[6 * j + i] = s;
        }
}

// rel[f * n_bundles + b] for every (f, b) below n_frames x n_bundles; cov NULL: status 2 for every posed pair
__global__ void __launch_bounds__(64) k_bundle_relative(const CamPoseRec *__restrict__ poses, const PoseCovRec *__restrict__ cov, int n_frames,
                                                        int n_bundles, int ref, BundleRelRec *__restrict__ rel)
{
    const long long i = (long long)blockIdx.x * ASL_WAVE + threadIdx.x, n = (long long)n_frames * n_bundles;
    if (i >= n) return;
    const int f = (int)(i / n_bundles), b = (int)(i - (long long)f * n_bundles);
    const size_t ia = (size_t)f * n_bundles + ref, ib = (size_t)i;
    const CamPoseRec *pa = poses + ia, *pb = poses + ib;
    BundleRelRec *o = rel + ib;
    o->reserved = 0;
    if (pa->status != 0 || pb->status != 0 || b == ref) {  // no pose (1), or the reference itself (0 or 1 by its pose)
#pragma unroll
        for (int k = 0; k < 16; k++) o->T[k] = (k % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 36; k++) o->cov[k] = 0.0;
        o->status = (pa->status != 0 || pb->status != 0) ? 1 : 0;
        return;
    }
    double Ra[9], Rb[9], Rab[9], ta[3], tb[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { Ra[3 * r + c] = pa->T[4 * r + c]; Rb[3 * r + c] = pb->T[4 * r + c]; }
        ta[r] = pa->T[4 * r + 3];
        tb[r] = pb->T[4 * r + 3];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rab[3 * r + c] = Ra[3 * r] * Rb[3 * c] + Ra[3 * r + 1] * Rb[3 * c + 1] + Ra[3 * r + 2] * Rb[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = Rab[3 * r] * tb[0] + Rab[3 * r + 1] * tb[1] + Rab[3 * r + 2] * tb[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o->T[4 * r] = Rab[3 * r]; o->T[4 * r + 1] = Rab[3 * r + 1]; o->T[4 * r + 2] = Rab[3 * r + 2];
        o->T[4 * r + 3] = ta[r] - q[r];
    }
    o->T[12] = 0; o->T[13] = 0; o->T[14] = 0; o->T[15] = 1;
    const bool have = cov && cov[ia].status == 0 && cov[ib].status == 0;
    if (!have) {
#pragma unroll
        for (int k = 0; k < 36; k++) o->cov[k] = 0.0;
        o->status = 2;
        return;
    }
    // C_a + D C_b D^T (symmetric from one computation), then the congruence with J_a
    double D[36], Ja[36], Cb[36], S[36];
#pragma unroll
    for (int k = 0; k < 36; k++) { D[k] = 0; Ja[k] = (k % 7 == 0) ? 1.0 : 0.0; Cb[k] = cov[ib].cov[k]; }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) { D[6 * r + c] = Rab[3 * r + c]; D[6 * (3 + r) + 3 + c] = Rab[3 * r + c]; }
    Ja[6 * 3 + 1] = -q[2]; Ja[6 * 3 + 2] = q[1];   // [q]x
    Ja[6 * 4 + 0] = q[2];  Ja[6 * 4 + 2] = -q[0];
    Ja[6 * 5 + 0] = -q[1]; Ja[6 * 5 + 1] = q[0];
    bundle_congruence(D, Cb, S);
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) {
            const double v = cov[ia].cov[6 * r + c] + S[6 * r + c];
            S[6 * r + c] = v;
            S[6 * c + r] = v;
        }
    bundle_congruence(Ja, S, o->cov);
    o->status = 0;
}
