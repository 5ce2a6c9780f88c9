// Locating unmapped tags from posed frames (asl_locate_tags_frames_device / asl_locate_tags_batch): the dual of
// k_localize.inc.  There one wavefront solves a frame's camera pose with the map held fixed; here one wavefront solves a
// tag's world<-tag pose G from all its views with the cameras held fixed.  Float64 throughout.  The result is not the joint
// optimum: the frame poses are taken as exact, as localisation takes the map as exact.
//   wanted  id i is solved for if its map entry has valid == 0 and a size that is >= 0 and finite (> 0: the tag's own side,
//           0: the call's tag_size; map_tag_half's rule).  Every other id gets status 1 and keeps its entry's bytes.
//   views   frame f takes part if poses[f].status is 0 or 6 and rows 0..2 of its T are finite; in such a frame every camera
//           c of the camera-major block obs[n_cams][n_frames][max_tags] gives at most one view of the tag, its first slot
//           with flags & 1 and id == i (one camera: n_cams = 1, the frame's view).  C = camera<-world of the view.
//   mark    k_locate_mark, one thread per slot: seen[id] = 1 for a wanted id with a view (every writer stores the same 1)
//   count   k_locate_count, one wavefront per seen id: the frames 64 at a time, lane = frame with its 0..n_cams views, a
//           wave sum
//   scan    k_locate_scan, one workgroup: ptr[n_ids + 1], the exclusive prefix of the counts (map_scan)
//   solve   one wavefront per id: fills its segment of the view list with frame * (n_cams * max_tags) + camera * max_tags +
//           slot in (frame, camera) order, each lane its frame's entries at the wave's exclusive prefix, then, corner
//           4 * view + q on lane % 64 and every sum a butterfly sum (the serial parts run redundantly in all lanes on
//           identical inputs, as in k_localize.inc):
//     seed    the <= 8 active views with flags & 2 of largest corner area (ties: lower list position), in list order, plain
//             before mirrored: G = inv(C_f) T_obs, a sized tag's PnP translation first times h_id / half, the mirror formed
//             in the camera frame; the strictly lowest total cost over ALL active views wins
//     refine  pose_lm on G, left update G <- [Rod(w) | v] G in the world frame: J = J_proj R_f [-[X_w]x | I]
//     gate    max_view_rms_px > 0: while the active view of largest own 4-corner RMS exceeds it, that view is dropped (one at
//             a time, at most 8, never the last) and the solve is RE-SEEDED: the start is the lowest-cost of the current pose
//             and the candidates of the views still active.  (k_localize continues from the current pose; a spoiled view
//             can pull a tag into its mirrored minimum, and from there the LM does not come back.)
//     cov     k_locate_solve<true>: one more linearisation at the pose written, lane c solves column c of
//             sigma^2 (J^T J)^-1 in the (r, d) convention of world<-tag (pose_cov_column_dev<false>); dof = 8 n_views - 6
// A view's C and corners are read from global memory in every pass (latency-bound scalar float64, not bytes).  No atomics,
// no host wait between the kernels: the same input gives the same bytes.  tests/locate_ref.py is the NumPy statement.
// The solve is one body, locate_solve_tag, over a view model, as loc_solve_frame is over LocOne / LocRig:
//   LocateOne  k_locate_solve: the frames' poses are world<-camera, C = inv(T_f), one CamDev in registers; no LDS
//   LocateRig  k_locate_solve_rig (asl_locate_tags_rig_*): the poses are world<-rig and camera c is mounted at E_c =
//              camera_c<-rig, C = E_c inv(T_f) = (Re R, Re t + te) formed where it is used; the camera table lies in LDS
//              (rig_fill_cams, published by a barrier) and a view's CamDev is built from its record there, so that no
//              per-camera choice becomes a run-time-indexed register array.  Seeding areas are pixels as they are.  A rig
//              of one camera with E = I is LocateOne: Re = I multiplies exactly.  tests/locate_rig_ref.py is its statement.

struct TagFitRec {  // == asl_tag_fit, 40 bytes
    double rms_px, rms_seed_px;
    int32_t n_views, n_rejected, status, seed_frame, seed_mirrored, reserved;
};

struct LocateArgs {
    const ObsRec *obs;  // [n_cams][n_frames][max_tags]; one camera: n_cams = 1
    int n_cams, n_frames, max_tags;
    const CamPoseRec *poses;
    MapTagRec *map;  // in / out
    int n_ids;
    int *seen, *cnt;  // per id
    int *ptr;         // n_ids + 1
    int *views;       // <= n_cams * n_frames * max_tags: frame * (n_cams * max_tags) + camera * max_tags + slot, by id, in
                      // (frame, camera) order
};

// Id wanted: valid == 0 and a size map_tag_half accepts; h: the tag's half side (comes in as the call's)
__device__ __forceinline__ bool locate_wanted(const MapTagRec &e, double &h)
{
    MapTagRec v;
    v.valid = 1;
    v.size = e.size;
    return !e.valid && map_tag_half(v, h);
}

// A frame takes part: a pose of the frame's own solve (0) or carried by the sequence prior (6), rows 0..2 finite
__device__ __forceinline__ bool locate_frame_ok(const CamPoseRec &p)
{
    if (p.status != 0 && p.status != 6) return false;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 12; i++) fin = fin && isfinite(p.T[i]);
    return fin;
}

// the slot of id's view in camera c's records of frame f (a frame that takes part), -1 without one
__device__ __forceinline__ int locate_view_slot(const LocateArgs &a, int f, int c, int id)
{
    const ObsRec *fo = a.obs + ((size_t)c * a.n_frames + f) * a.max_tags;
    for (int s = 0; s < a.max_tags; s++)
        if ((fo[s].flags & 1) && fo[s].id == id) return s;
    return -1;
}

// The views of id in frame f, one per camera at most: their number, the cameras as a bit mask, camera c's slot in byte c of
// (lo, hi) (a slot is below 256; two words chosen by a compare, not an array indexed by c)
struct LocateFrameViews {
    unsigned long long lo, hi;
    unsigned int cams;
    int n;
    __device__ __forceinline__ int slot(int c) const { return (int)(((c < 8 ? lo : hi) >> (8 * (c & 7))) & 255ull); }
};

__device__ __forceinline__ LocateFrameViews locate_frame_views(const LocateArgs &a, int f, int id)
{
    LocateFrameViews v{0ull, 0ull, 0u, 0};
    if (f >= a.n_frames || !locate_frame_ok(a.poses[f])) return v;
    for (int c = 0; c < a.n_cams; c++) {
        const int s = locate_view_slot(a, f, c, id);
        if (s < 0) continue;
        const unsigned long long b = (unsigned long long)s << (8 * (c & 7));
        if (c < 8) v.lo |= b;
        else v.hi |= b;
        v.cams |= 1u << c;
        v.n++;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_locate_mark(LocateArgs a)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)a.n_cams * (size_t)a.n_frames * (size_t)a.max_tags) return;
    const int id = a.obs[k].id;
    if (!(a.obs[k].flags & 1) || id < 0 || id >= a.n_ids) return;
    double h = 0;
    if (!locate_wanted(a.map[id], h) || !locate_frame_ok(a.poses[(k / (size_t)a.max_tags) % (size_t)a.n_frames])) return;
    a.seen[id] = 1;
}

__global__ void __launch_bounds__(64) k_locate_count(LocateArgs a)
{
    const int i = blockIdx.x, lane = threadIdx.x;
    int n = 0;
    if (a.seen[i]) {
        for (int f0 = 0; f0 < a.n_frames; f0 += ASL_WAVE) {
            int tot;
            wave_prefix_sum(locate_frame_views(a, f0 + lane, i).n, &tot);
            n += tot;
        }
    }
    if (lane == 0) a.cnt[i] = n;
}

__global__ void __launch_bounds__(MAP_WG) k_locate_scan(LocateArgs a)
{
    __shared__ int s_part[MAP_WG + 1];
    map_scan(a.n_ids, [&](int i) { return a.cnt[i]; }, s_part, a.ptr);
}

// inv(T_f) of frame f (R row-major 9, t 3), formed from the record: camera<-world of one camera, rig<-world of a rig
__device__ __forceinline__ void locate_frame_inv(const LocateArgs &a, int f, double *C)
{
    const double *T = a.poses[f].T;
    double W[12];
#pragma unroll
    for (int r = 0; r < 3; r++) { W[3 * r] = T[4 * r]; W[3 * r + 1] = T[4 * r + 1]; W[3 * r + 2] = T[4 * r + 2]; W[9 + r] = T[4 * r + 3]; }
    pk_inv(W, C);
}

// A view entry taken apart: its frame, its record and (a rig) its camera's LDS record
struct LocateView {
    int frame;
    const ObsRec *rec;
    const double *cl;
};

// The view model of one camera: entry e is record e of the block, every view goes through the one CamDev
struct LocateOne {
    CamDev cam;
    __device__ __forceinline__ LocateView view(const LocateArgs &a, int e) const { return {e / a.max_tags, a.obs + e, nullptr}; }
    __device__ __forceinline__ void view_cam(const LocateArgs &a, const LocateView &v, double *C) const { locate_frame_inv(a, v.frame, C); }
    __device__ __forceinline__ CamDev cam_of(const LocateView &) const { return cam; }
};

// The view model of a rig: entry e = f * (n_cams * max_tags) + g with the global slot g = c * max_tags + s of k_rig.inc,
// the record obs[c][f][s], camera<-world C = E_c inv(T_f) (LocRig::camera_pose's formula) and the CamDev of camera c's LDS
// record (rig_cam_dev)
struct LocateRig {
    const double *cams;  // LDS: RIG_CAM_DOUBLES per camera
    unsigned int magic;
    __device__ __forceinline__ LocateView view(const LocateArgs &a, int e) const
    {
        const int ns = a.n_cams * a.max_tags, f = e / ns, g = e - f * ns, c = rig_cam_of(g, magic);
        return {f, a.obs + ((size_t)c * a.n_frames + f) * a.max_tags + (g - c * a.max_tags), cams + RIG_CAM_DOUBLES * c};
    }
    __device__ __forceinline__ void view_cam(const LocateArgs &a, const LocateView &v, double *C) const
    {
        const double *Re = v.cl + 9, *te = v.cl + 18;
        double W[12];
        locate_frame_inv(a, v.frame, W);
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int k = 0; k < 3; k++) C[3 * i + k] = Re[3 * i] * W[k] + Re[3 * i + 1] * W[3 + k] + Re[3 * i + 2] * W[6 + k];
            C[9 + i] = Re[3 * i] * W[9] + Re[3 * i + 1] * W[10] + Re[3 * i + 2] * W[11] + te[i];
        }
    }
    __device__ __forceinline__ CamDev cam_of(const LocateView &v) const { return rig_cam_dev(v.cl); }
};

// Squared pixel error of corner q of a tag of half side h at world<-tag (R, t), seen through camera<-world C at cf; with NE
// its rows of d uv / d (w, v) = J_proj R_C [-[X_w]x | I] are added to acc (map_tag_pass's formula)
template <bool NE>
__device__ __forceinline__ double locate_corner(const CamDev &cam, const double *C, const float *cf, double h, const double *R, const double *t,
                                                int q, double *acc)
{
    const double ox = (q == 1 || q == 2) ? h : -h, oy = (q >= 2) ? h : -h;
    double X[3], P[3], uv[2], Jp[6];
#pragma unroll
    for (int r = 0; r < 3; r++) X[r] = R[3 * r] * ox + R[3 * r + 1] * oy + t[r];
#pragma unroll
    for (int r = 0; r < 3; r++) P[r] = C[3 * r] * X[0] + C[3 * r + 1] * X[1] + C[3 * r + 2] * X[2] + C[9 + r];
    if (!(P[2] > LOC_Z_MIN)) return LOC_BEHIND_COST;
    project_dev(cam, P, uv, NE ? Jp : nullptr);
    const double r0 = uv[0] - (double)cf[2 * q], r1 = uv[1] - (double)cf[2 * q + 1];
    if constexpr (NE) {
        double a0[3], a1[3], J0[6], J1[6];  // a = J_proj R_C: d uv / d X_world
#pragma unroll
        for (int k = 0; k < 3; k++) {
            a0[k] = Jp[0] * C[k] + Jp[1] * C[3 + k] + Jp[2] * C[6 + k];
            a1[k] = Jp[3] * C[k] + Jp[4] * C[3 + k] + Jp[5] * C[6 + k];
        }
        J0[0] = X[1] * a0[2] - X[2] * a0[1]; J0[1] = X[2] * a0[0] - X[0] * a0[2]; J0[2] = X[0] * a0[1] - X[1] * a0[0];
        J1[0] = X[1] * a1[2] - X[2] * a1[1]; J1[1] = X[2] * a1[0] - X[0] * a1[2]; J1[2] = X[0] * a1[1] - X[1] * a1[0];
#pragma unroll
        for (int k = 0; k < 3; k++) { J0[3 + k] = a0[k]; J1[3 + k] = a1[k]; }
#pragma unroll
        for (int p = 0; p < 6; p++) {
            acc[21 + p] += J0[p] * r0 + J1[p] * r1;
#pragma unroll
            for (int p2 = 0; p2 <= p; p2++) acc[TRI(p, p2)] += J0[p] * J0[p2] + J1[p] * J1[p2];
        }
    }
    return r0 * r0 + r1 * r1;
}

// The views the gate dropped, by list position (-1: none): registers, the same in every lane
struct LocateDrops {
    int o[LOC_MAX_GATE_DROPS];
    __device__ __forceinline__ bool has(int v) const
    {
        bool d = false;
#pragma unroll
        for (int r = 0; r < LOC_MAX_GATE_DROPS; r++) d = d || o[r] == v;
        return d;
    }
    __device__ __forceinline__ void add(int k, int v)
    {
#pragma unroll
        for (int r = 0; r < LOC_MAX_GATE_DROPS; r++)
            if (r == k) o[r] = v;
    }
};

// Total corner cost of world<-tag (R, t) over the active views of the n at list offset b, identical in every lane; with NE
// also the normal equations of the tag's left update (packed lower triangle 21, then J^T r 6)
template <bool NE, class M>
__device__ __forceinline__ double locate_pass(const M &m, const LocateArgs &a, double h, int b, int n, const LocateDrops &drops,
                                              const double *R, const double *t, int lane, double *ne)
{
    double cost = 0, acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0;
    for (int k = lane; k < 4 * n; k += ASL_WAVE) {
        const int o = k >> 2;
        if (drops.has(o)) continue;
        const LocateView v = m.view(a, a.views[b + o]);
        double C[12];
        m.view_cam(a, v, C);
        cost += locate_corner<NE>(m.cam_of(v), C, v.rec->corners, h, R, t, k & 3, acc);
    }
    if constexpr (NE) {
#pragma unroll
        for (int i = 0; i < 27; i++) ne[i] = butterfly_sum<64>(acc[i]);
    }
    return butterfly_sum<64>(cost);
}

// an id without a pose: its fit record, and its covariance record if there is one
__device__ __forceinline__ void locate_write_none(TagFitRec *o, PoseCovRec *oc, double sigma_px, int status, int n_views, int lane)
{
    if (lane == 0) {
        o->rms_px = 0; o->rms_seed_px = 0; o->n_views = n_views; o->n_rejected = 0; o->status = status; o->seed_frame = -1;
        o->seed_mirrored = 0; o->reserved = 0;
    }
    if (oc) loc_cov_write_none(oc, sigma_px, lane);
}

// One id's solve by one wavefront over the view model vm (LocateOne, LocateRig): the one copy of list fill, seed, refine,
// gate and covariance.  half: the call's tag_size / 2.  COV: also *oc, which the plain instantiations never touch
template <bool COV, class M>
__device__ __forceinline__ void locate_solve_tag(const M &vm, const LocateArgs &a, int i, double half, double gate, int min_views, TagFitRec *o,
                                                 PoseCovRec *oc, double sigma_px, int lane)
{
    double h = half;
    if (!locate_wanted(a.map[i], h)) { locate_write_none(o, oc, sigma_px, 1, 0, lane); return; }

    // the view list of this id, in (frame, camera) order, then visible to the whole wave
    const int b = a.ptr[i], cap = a.ptr[i + 1] - b;
    int n = 0;
    if (a.seen[i]) {
        for (int f0 = 0; f0 < a.n_frames; f0 += ASL_WAVE) {
            const int f = f0 + lane;
            const LocateFrameViews fv = locate_frame_views(a, f, i);
            int tot, pos = n + wave_prefix_sum(fv.n, &tot);
            for (int c = 0; c < a.n_cams; c++) {
                if (!((fv.cams >> c) & 1u)) continue;
                if (pos < cap) a.views[b + pos] = (f * a.n_cams + c) * a.max_tags + fv.slot(c);  // cap: what k_locate_count found
                pos++;
            }
            n += tot;
        }
        n = min(n, cap);
        // the list goes back through this CU's L1, which may hold a neighbouring id's part of a line from before the
        // stores: an agent-scope fence (write back, then invalidate), its stores drained, before any lane reads
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (n < min_views) { locate_write_none(o, oc, sigma_px, 2, n, lane); return; }

    const double ks = map_seed_scale(h, half);
    LocateDrops drops;
#pragma unroll
    for (int r = 0; r < LOC_MAX_GATE_DROPS; r++) drops.o[r] = -1;
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return locate_pass<decltype(ne_tag)::value>(vm, a, h, b, n, drops, R, t, lane, ne);
    };
    auto score = [&](const double *P) { return locate_pass<false>(vm, a, h, b, n, drops, P, P + 9, lane, nullptr); };

    double P[12], cost = 0, best = INFINITY, best_first = 0;
    int nused = n, nrej = 0, seed_frame = -1, seed_mirrored = 0;
    for (;;) {
        // seed: the <= 8 active seeding views of largest area, every candidate in list order, plain before mirrored; after
        // a drop the current pose is candidate 0
        if (nrej > 0) best = score(P);
        int sel[LOC_MAX_SEEDS];
        const int nsel = loc_top_k(n, lane, [&](int v) {
            if (drops.has(v)) return -1.0;
            const ObsRec *rec = vm.view(a, a.views[b + v]).rec;
            return (rec->flags & 2) ? loc_area(rec->corners) : -1.0;
        }, sel);
        int won = -1, wm = 0, prev = -1;
        for (int j = 0; j < nsel; j++) {
            int v = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < LOC_MAX_SEEDS; r++)
                if (sel[r] > prev && sel[r] < v) v = sel[r];
            prev = v;
            const LocateView sv = vm.view(a, a.views[b + v]);
            double C[12], Wi[12];
            vm.view_cam(a, sv, C);
            pk_inv(C, Wi);
            for (int m = 0; m < 2; m++) {
                double A[12], G[12];
                map_obs_pose(*sv.rec, ks, m == 1, A);
                pk_mul(Wi, A, G);
                const double c = score(G);
                if (c < best) {
                    best = c; won = v; wm = m;
#pragma unroll
                    for (int k = 0; k < 12; k++) P[k] = G[k];
                }
            }
        }
        if (nrej == 0) {
            if (won < 0) { locate_write_none(o, oc, sigma_px, 3, n, lane); return; }  // no seeding view, or every score NaN
            best_first = best;
            seed_frame = vm.view(a, a.views[b + won]).frame;
            seed_mirrored = wm;
        }

        // refine
        cost = pose_lm(pass, P, P + 9);

        // gate: the worst active view, if it is over the gate, goes
        if (!(gate > 0) || nrej >= LOC_MAX_GATE_DROPS || nused <= 1) break;
        double wr = -1.0;
        int wv = 0x7fffffff;
        for (int v = lane; v < n; v += ASL_WAVE) {
            if (drops.has(v)) continue;
            const LocateView gv = vm.view(a, a.views[b + v]);
            const CamDev cam = vm.cam_of(gv);
            double C[12], eq[4];
            vm.view_cam(a, gv, C);
#pragma unroll
            for (int q = 0; q < 4; q++) eq[q] = locate_corner<false>(cam, C, gv.rec->corners, h, P, P + 9, q, nullptr);
            const double rms = sqrt(((eq[0] + eq[1]) + (eq[2] + eq[3])) / 4);
            if (rms > wr) { wr = rms; wv = v; }
        }
        argmax_step<1>(wr, wv); argmax_step<2>(wr, wv); argmax_step<4>(wr, wv);
        argmax_step<8>(wr, wv); argmax_step<16>(wr, wv); argmax_step<32>(wr, wv);
        if (!(wr > gate)) break;
        drops.add(nrej, wv);
        nrej++;
        nused--;
    }

    // the extended map's entry (size kept) and the fit
    if (lane == 0) {
        pk_to34(P, a.map[i].T);
        a.map[i].valid = 1;
        o->rms_px = sqrt(cost / (4.0 * nused));
        o->rms_seed_px = sqrt(best_first / (4.0 * n));
        o->n_views = nused; o->n_rejected = nrej; o->status = 0; o->seed_frame = seed_frame; o->seed_mirrored = seed_mirrored;
        o->reserved = 0;
    }

    // the covariance at the pose just written, as loc_solve_frame<true> does: world<-tag is the pose solved for itself
    if constexpr (COV) {
        double ne[27], col[6], sig;
        const double c1 = locate_pass<true>(vm, a, h, b, n, drops, P, P + 9, lane, ne);
        const int dof = 8 * nused - 6;
        const double s2 = pose_cov_sigma2(sigma_px, c1, dof, &sig);
        const int c = lane < 6 ? lane : 5;
        const bool pd = pose_cov_column_dev<false>(ne, P, P + 9, c, col) && isfinite(s2);
        if (lane < 6) pose_cov_store_column(oc, c, col, s2, pd);
        if (lane == 36) oc->sigma_px = sig;
        if (lane == 37) { oc->dof = dof; oc->status = pd ? 0 : 2; }
    }
}

// One wavefront per id, one camera; COV: also cov[id]
template <bool COV>
__global__ void __launch_bounds__(64) k_locate_solve(LocateArgs a, CamDev cam, double gate, int min_views, TagFitRec *__restrict__ fit,
                                                     PoseCovRec *__restrict__ cov, double sigma_px)
{
    const int i = blockIdx.x;
    locate_solve_tag<COV>(LocateOne{cam}, a, i, cam.half, gate, min_views, fit + i, COV ? cov + i : nullptr, sigma_px, (int)threadIdx.x);
}

// One wavefront per id, a rig: the camera table to LDS first, published by the barrier before the solve reads it
template <bool COV>
__global__ void __launch_bounds__(64) k_locate_solve_rig(LocateArgs a, const RigCamRec *__restrict__ rig, double half, double gate, int min_views,
                                                         TagFitRec *__restrict__ fit, PoseCovRec *__restrict__ cov, double sigma_px)
{
    __shared__ double s_cams[RIG_MAX_CAMS * RIG_CAM_DOUBLES];
    const int i = blockIdx.x, lane = threadIdx.x;
    rig_fill_cams(s_cams, rig, a.n_cams, lane);
    __syncthreads();
    locate_solve_tag<COV>(LocateRig{s_cams, 65536u / (unsigned int)a.max_tags + 1u}, a, i, half, gate, min_views, fit + i, COV ? cov + i : nullptr,
                          sigma_px, lane);
}
