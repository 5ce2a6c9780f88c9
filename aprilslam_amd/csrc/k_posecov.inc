// Per-tag pose covariance (asl_pose_cov_device / asl_solve_pnp_cov_batch): the first-order covariance of the camera<-tag
// pose an asl_obs record holds, from its 4 corners.  A quad of lanes per record as the PnP has it (k_pnp.inc), lane q of
// the quad = corner q, float64 throughout: each lane linearises its own corner at the record's pose with loc_corner<true>
// (k_localize.inc: project_dev and the Jacobian of the left update), butterfly_sum<4> adds the 21 + 6 + 1 sums over the
// quad (the same bits in its four lanes), and the six columns of the covariance (pose_cov_column_dev, k_pnp.inc) are
// solved two rounds deep: lane q column q, then lanes 0 and 1 columns 4 and 5.  No LDS, no loop of data-dependent length:
// every record costs the same, so 16 records fill a wave without the PnP's tail.  It lives here and not in k_pnp.inc
// because ObsRec and loc_corner come later in the include order.

__global__ void __launch_bounds__(64) k_pnp_cov(const ObsRec *__restrict__ obs, int n, CamDev cam, double sigma_px, PoseCovRec *__restrict__ cov)
{
    const int lane = threadIdx.x, gi = lane >> 2, q = lane & 3;
    const int i = blockIdx.x * PNP_TAGS_PER_WAVE + gi;
    const bool have = i < n;
    const bool posed = have && (obs[have ? i : 0].flags & 2) != 0;  // the DPP sums need every lane of the quad: others linearise a dummy
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 1}, iu = cam.cx, iv = cam.cy;
    if (posed) {
        const ObsRec *o = obs + i;
#pragma unroll
        for (int r = 0; r < 3; r++) { R[3 * r] = o->T[4 * r]; R[3 * r + 1] = o->T[4 * r + 1]; R[3 * r + 2] = o->T[4 * r + 2]; t[r] = o->T[4 * r + 3]; }
        iu = (double)o->corners[2 * q];
        iv = (double)o->corners[2 * q + 1];
    }
    const double X[3] = {(q == 1 || q == 2) ? cam.half : -cam.half, (q >= 2) ? cam.half : -cam.half, 0.0};
    double acc[27], ne[21];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0;
    const double cost = butterfly_sum<4>(loc_corner<true>(cam, R, t, X, iu, iv, acc));
#pragma unroll
    for (int k = 0; k < 21; k++) ne[k] = butterfly_sum<4>(acc[k]);
    double sig, col[6];
    const double s2 = pose_cov_sigma2(sigma_px, cost, 2, &sig);
    bool pd = pose_cov_column_dev<false>(ne, R, t, q, col) && isfinite(s2);
    if (!have) return;
    PoseCovRec *oc = cov + i;
    pose_cov_store_column(oc, q, col, s2, posed && pd);
    if (q < 2) {
        pd = pose_cov_column_dev<false>(ne, R, t, 4 + q, col) && pd;
        pose_cov_store_column(oc, 4 + q, col, s2, posed && pd);
    } else if (q == 2)
        oc->sigma_px = posed ? sig : sigma_px;
    else {
        oc->dof = posed ? 2 : 0;
        oc->status = posed ? (pd ? 0 : 2) : 1;
    }
}
