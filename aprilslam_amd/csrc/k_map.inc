// Tag-map reconstruction from a batch of frames (asl_map_frames_device / asl_map_batch): world<-tag poses of every tag
// the frames see, each frame's camera pose and a per-tag std, from the asl_obs block alone.  float64 throughout;
// tests/map_ref.py is the NumPy statement of the same computation.
//   k_map_gather    one workgroup: taking-part slots, used frames (>= 2 slots of distinct ids) -> cameras, ids seen -> tags
//                   (ascending), observations in (frame, slot) order, the world tag; the host reads the sizes (its one wait)
//   k_map_csr       one workgroup: the (camera, tag) -> first active observation table k_gn_schur reads, each pair's chain
//                   of later ones, and the per-camera and per-tag lists of the active observations (in observation
//                   order); run after each stage that drops
//   k_map_chain     one workgroup: breadth-first rounds from the world tag (cameras, then tags, each half reading the state
//                   the previous one left) -- map_init.chain_initial_map without its dependence on frame order
//   k_map_sweep_cam per camera (one wavefront): reseed_poses' camera half -- k_localize.inc's slot gather, top-8 choice,
//                   candidates (loc_candidate) and scoring (loc_pass) against the current map, the current pose as candidate 0
//   k_map_sweep_tag per tag (one wavefront): the dual, the cameras held; candidate poses inv(W) T_obs and its mirror
//   k_map_gauge     one workgroup: the world tag back at the identity
//   k_map_flip      per tag: the pose and its mirror (built in the view of largest area) each polished by pose-only LM
//                   (k_localize.inc: pose_lm)
//   k_map_behind    per camera: observations with a corner at z <= 1e-6 leave; a camera left with < 2 is dropped
//   then gn_host.inc's LM loop (gn_lm_run: k_gn.inc's reduced system, Cholesky, step, cost and commit) with
//   k_map_linearize (k_gn.inc's gn_obs_block with the lens model), k_map_decide (gn_accept, and the stop rule) and, after
//   each trial, k_map_park: after the stop it empties the LM's copy of the list offsets, so that the remaining trials
//   reduce and factor an identity system;
//   k_map_std       per tag parameter: diag of S^-1 = |L^-1 e_i|^2 by blocked forward substitution with the factor
//                   (the covariance calls, asl_mapcov_* / asl_mapcov_rig_*: k_map_cols keeps the columns, and after
//                   k_map_finish k_map_cov_gram forms s^2 S^-1 over the tags k_map_finish numbered)
//   k_map_finish    one workgroup: the records.
// The robust calls (asl_map_robust_*, huber_px = k > 0; tests/map_ref.py "loss") keep every seeding stage as it is and put
// a Huber loss on each corner's raw residual in the LM alone: k_map_linearize<true> scales a corner's two rows by
// sqrt(weight) and costs it 2 k s - k^2 beyond k, so gn_obs_block, the reduced system and the accept rule see a weighted
// problem and the D blocks the std reads are weighted already.  After the LM
//   k_map_soft      one workgroup: per observation the smallest corner weight at the committed poses; the number of soft
//                   observations, the squared error and the number of the corners not over k, summed in a fixed order
// which k_map_finish takes for n_soft, the slot weights and the std's variance factor.  huber_px = 0 runs the plain kernels.
// A camera rig (asl_map_rig_*, tests/map_ref.py "block"): the block is camera-major, obs[n_rig][n_frames][max_tags], the
// "cameras" of the joint problem are the used rig frames with W = rig<-world, and an observation is a VIEW, a taking-part
// slot of one rig camera, in (frame, camera, slot) order.  The kernels are written once over the view's camera
// (map_view<RIG>): one camera is the call's model and W itself, a rig the table's entry (a.cams, k_rig.inc's layout, read
// where it is used) and E_c W.  A (frame, tag) pair may have several views; the seeding, k_map_soft, the behind test and
// the records work on the view lists (a.tag_ptr / a.tag_obs), the reduced system on the pair lists (a.cam_*, a.ptag_*,
// a.obs_of), which hold the pair's first active view.  12 x 13 blocks of views of one pair are additive, so after each
// linearisation k_map_fold adds the later views' blocks to the first one's, in view order (a.obs_next).  With one camera
// every pair has one view, the two sets of lists are equal and nothing is folded.
// Tags of different sizes (asl_map_*sized*, tests/map_ref.py "sizes"): the caller's per-id table (a.sizes; all 0 in every
// other call) gives each tag its half side (a.tag_half, k_map_gather; map_tag_half's rule), which every pass that forms a
// tag's corners reads in place of the call's, and a sized tag's PnP translation is multiplied by h / half wherever a
// record proposes a pose (map_seed_scale: the chain, both sweeps' candidates).  Sizes are given, never solved for.
// No atomics: every sum has a fixed order (wave butterflies, per-thread loops in list order, k_gn_cost's fixed tree), so the
// same input gives the same bytes; frames without taking-part slots change no list, no index and no sum.

struct MapResultRec {  // == asl_map_result, 64 bytes
    double cost_seed, cost, rms_px, rms_seed_px;
    int32_t n_frames_used, n_tags, n_obs, n_obs_dropped, iterations, world_id, status, n_soft;
};

struct MapHead {  // the sizes the host reads once
    int n_cams, n_tags, n_obs, world_tag, world_id, n_act, pad0, pad1;
};

#define MAP_WG 1024
#define MAP_MAX_CAND 8
#define MAP_BEHIND_MARGIN 1e-6
#define MAP_MAX_TAGS 1000
#define MAP_MAX_ITERS 1000  // every trial is enqueued up front (the host does not wait for the stop)
// LM state beyond k_gn.inc's GN_LM__N entries (the k_gn kernels read only those)
enum { MAP_LM_STOP = GN_LM__N, MAP_LM_ITERS, MAP_LM_STATUS, MAP_LM__N = 16 };

struct MapArgs {
    const ObsRec *obs;
    int n_frames, max_tags, n_ids, world_req;
    int n_rig;                                              // cameras a frame has: 1, or the rig's
    const double *cams;                                     // a rig: RIG_CAM_DOUBLES per camera (k_rig.inc's layout)
    MapHead *head;
    int *seen, *id_tag, *tag_id, *tmp, *tmp2;               // per id (n_ids + 1)
    int *fr_npart, *fr_ndist, *fr_cam, *fr_obs0;            // per frame (+1): taking-part slots, distinct ids among them
    int *cam_frame, *cam_ptr0, *cam_state, *cam_seed;       // per camera (<= n_frames, +1)
    int *tag_state;                                         // per tag (<= n_ids)
    int *slot_obs;                                          // per slot of the block
    int *obs_slot, *obs_cam, *obs_tag, *obs_act;            // per observation (<= n_rig * n_frames * max_tags); obs_slot: in the block
    int *tag_ptr, *tag_obs;                                 // every active observation by tag
    int *cam_ptr, *cam_obs, *ptag_ptr, *ptag_obs, *obs_of;  // the first active one of each (camera, tag) pair: lists and table
    int *obs_next;                                          // the pair's next active observation, -1 at the end
    double *W, *G;                                          // camera<-world, world<-tag: R row-major (9), t (3)
    const float *sizes;                                     // per id: the tag's own side, 0: the call's tag_size (all 0 without a table)
    double *tag_half;                                       // per tag: its half side (k_map_gather); the call's half for size 0
};

// ---- small helpers on 12-double poses
__device__ __forceinline__ void pk_mul(const double *A, const double *B, double *C)
{
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
        C[9 + r] = A[3 * r] * B[9] + A[3 * r + 1] * B[10] + A[3 * r + 2] * B[11] + A[9 + r];
    }
}

__device__ __forceinline__ void pk_inv(const double *A, double *B)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) B[3 * r + c] = A[3 * c + r];
#pragma unroll
    for (int r = 0; r < 3; r++) B[9 + r] = -(B[3 * r] * A[9] + B[3 * r + 1] * A[10] + B[3 * r + 2] * A[11]);
}

__device__ __forceinline__ void pk_eye(double *A)
{
#pragma unroll
    for (int i = 0; i < 12; i++) A[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
}

// 12-double pose -> rows 0..2 of a 4x4 (asl_obs.T, asl_map_tag.T)
__device__ __forceinline__ void pk_to34(const double *A, double *T)
{
#pragma unroll
    for (int r = 0; r < 3; r++) { T[4 * r] = A[3 * r]; T[4 * r + 1] = A[3 * r + 1]; T[4 * r + 2] = A[3 * r + 2]; T[4 * r + 3] = A[9 + r]; }
}

// What a record's PnP pose, solved at the call's half, is for a tag of half side h: the rotation holds and the translation
// is short by half / h (k_localize.inc: loc_solve_frame).  1 exactly for a tag without a size, which takes the unscaled path.
__device__ __forceinline__ double map_seed_scale(double h, double half) { return h == half ? 1.0 : h / half; }

__device__ __forceinline__ void map_scale_obs(double *To, double k)
{
    if (k != 1.0) { To[3] *= k; To[7] *= k; To[11] *= k; }
}

// camera<-tag of a slot's PnP pose with its translation times k (map_seed_scale), or the mirrored planar minimum of that
// (loc_candidate against the identity)
__device__ __forceinline__ void map_obs_pose(const ObsRec &o, double k, bool mirror, double *A)
{
    double To[12], I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, R[9], t[3];
#pragma unroll
    for (int i = 0; i < 12; i++) To[i] = o.T[i];
    map_scale_obs(To, k);
    loc_candidate(To, I34, mirror, R, t);
#pragma unroll
    for (int i = 0; i < 9; i++) A[i] = R[i];
    A[9] = t[0]; A[10] = t[1]; A[11] = t[2];
}

// the rig camera of observation m (0 with one camera), and its entry of the rig's table
__device__ __forceinline__ int map_view_rig_cam(const MapArgs &a, int m) { return a.obs_slot[m] / (a.n_frames * a.max_tags); }
__device__ __forceinline__ const double *map_view_entry(const MapArgs &a, int m) { return a.cams + RIG_CAM_DOUBLES * map_view_rig_cam(a, m); }

// The camera of observation m: its model cv and its pose Wv = camera<-world where the frame's pose is W.  One camera: the
// call's model and W itself; a rig: the table's entry and E_c W (W = rig<-world).
template <bool RIG>
__device__ __forceinline__ void map_view(const MapArgs &a, const CamDev &cam, int m, const double *W, CamDev &cv, double *Wv)
{
    cv = cam;
    if constexpr (RIG) {
        const double *cl = map_view_entry(a, m);
        cv.fx = cl[0]; cv.fy = cl[1]; cv.cx = cl[2]; cv.cy = cl[3]; cv.k1 = cl[4]; cv.k2 = cl[5]; cv.p1 = cl[6]; cv.p2 = cl[7]; cv.k3 = cl[8];
        double Wr[12];
#pragma unroll
        for (int i = 0; i < 12; i++) Wr[i] = W[i];
        pk_mul(cl + 9, Wr, Wv);
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) Wv[i] = W[i];
    }
}

// a rig's table in k_rig.inc's layout, into a.cams: one wavefront
__global__ void __launch_bounds__(64) k_map_rig_table(double *cams, const RigCamRec *__restrict__ rig, int n_cams)
{
    rig_fill_cams(cams, rig, n_cams, (int)threadIdx.x);
}

// exclusive prefix sum of cnt(i), i < n, by the MAP_WG threads (contiguous chunks, then the chunks in order) into out[0..n]
// (if out); returns the total in every thread
template <class Cnt>
__device__ __forceinline__ int map_scan(int n, Cnt cnt, int *s_part, int *out)
{
    const int tid = threadIdx.x, per = (n + MAP_WG - 1) / MAP_WG;
    const int i0 = min(n, tid * per), i1 = min(n, i0 + per);
    int c = 0;
    for (int i = i0; i < i1; i++) c += cnt(i);
    s_part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < MAP_WG; i++) { const int v = s_part[i]; s_part[i] = run; run += v; }
        s_part[MAP_WG] = run;
    }
    __syncthreads();
    if (out) {
        int o = s_part[tid];
        for (int i = i0; i < i1; i++) { out[i] = o; o += cnt(i); }
        if (tid == 0) out[n] = s_part[MAP_WG];
    }
    const int total = s_part[MAP_WG];
    __syncthreads();
    return total;
}

// ---- gather: one workgroup.  half: the call's; a tag's own is map_tag_half's (double)(size * 0.5f)
__global__ void __launch_bounds__(MAP_WG) k_map_gather(MapArgs a, double half)
{
    __shared__ int s_part[MAP_WG + 1];
    const int tid = threadIdx.x, S = a.max_tags, NR = a.n_rig;
    auto slot = [&](int r, int f, int s) { return ((size_t)r * a.n_frames + f) * S + s; };  // the block is camera-major
    for (int i = tid; i < a.n_ids; i += MAP_WG) a.seen[i] = 0;
    for (int f = tid; f < a.n_frames; f += MAP_WG) {
        int np = 0, nd = 0;
        for (int r = 0; r < NR; r++) {
            const ObsRec *fo = a.obs + slot(r, f, 0);
            for (int s = 0; s < S; s++) {
                const int id = fo[s].id;
                bool p = (fo[s].flags & 1) && id >= 0 && id < a.n_ids;
                for (int s2 = 0; p && s2 < s; s2++)  // a repeated id takes part once per camera, in its first slot
                    if ((fo[s2].flags & 1) && fo[s2].id == id) p = false;
                a.slot_obs[slot(r, f, s)] = p ? 1 : -1;
                np += p;
                bool first = p;  // the frame's first view of the id: no earlier camera has one
                for (int k2 = 0; first && k2 < r * S; k2++)
                    if (a.slot_obs[slot(k2 / S, f, k2 % S)] == 1 && a.obs[slot(k2 / S, f, k2 % S)].id == id) first = false;
                nd += first;
            }
        }
        a.fr_npart[f] = np;
        a.fr_ndist[f] = nd;
    }
    __syncthreads();
    for (int f = tid; f < a.n_frames; f += MAP_WG) {
        if (a.fr_ndist[f] < 2) continue;
        for (int k = 0; k < NR * S; k++)
            if (a.slot_obs[slot(k / S, f, k % S)] == 1) a.seen[a.obs[slot(k / S, f, k % S)].id] = 1;  // every writer stores the same 1
    }
    __syncthreads();
    const int n_cams = map_scan(a.n_frames, [&](int f) { return a.fr_ndist[f] >= 2 ? 1 : 0; }, s_part, a.fr_cam);
    const int n_obs = map_scan(a.n_frames, [&](int f) { return a.fr_ndist[f] >= 2 ? a.fr_npart[f] : 0; }, s_part, a.fr_obs0);
    const int n_tags = map_scan(a.n_ids, [&](int i) { return a.seen[i]; }, s_part, a.id_tag);
    for (int f = tid; f < a.n_frames; f += MAP_WG) {
        const bool used = a.fr_ndist[f] >= 2;
        const int c = a.fr_cam[f];
        int m = a.fr_obs0[f];
        if (used) { a.cam_frame[c] = f; a.cam_ptr0[c] = m; }
        for (int g = 0; g < NR * S; g++) {  // (camera, slot) order
            const size_t k = slot(g / S, f, g % S);
            if (used && a.slot_obs[k] == 1) {
                a.obs_slot[m] = (int)k; a.obs_cam[m] = c; a.obs_tag[m] = a.id_tag[a.obs[k].id]; a.obs_act[m] = 1;
                a.slot_obs[k] = m++;
            } else
                a.slot_obs[k] = -1;
        }
    }
    for (int i = tid; i < a.n_ids; i += MAP_WG)
        if (a.seen[i]) {
            const float sz = a.sizes[i];
            a.tag_id[a.id_tag[i]] = i;
            a.tag_half[a.id_tag[i]] = sz > 0.0f ? (double)(sz * 0.5f) : half;
        }
    __syncthreads();
    if (tid == 0) {
        a.cam_ptr0[n_cams] = n_obs;
        int wt = -1, wid = a.world_req;
        if (a.world_req < 0) { if (n_tags > 0) { wt = 0; wid = a.tag_id[0]; } }
        else if (a.world_req < a.n_ids && a.seen[a.world_req]) wt = a.id_tag[a.world_req];
        MapHead h = {n_cams, n_tags, n_obs, wt, wid, 0, 0, 0};
        *a.head = h;
    }
}

// ---- active lists: one workgroup.  The table entry of a (camera, tag) pair is its first active observation, and obs_next
// chains the pair's later ones in observation order (one camera: there are none).  The tag lists walk the table in camera
// order and each chain, which is observation order.
__global__ void __launch_bounds__(MAP_WG) k_map_csr(MapArgs a, int n_cams, int n_tags)
{
    __shared__ int s_part[MAP_WG + 1];
    const int tid = threadIdx.x;
    for (size_t i = tid; i < (size_t)n_cams * n_tags; i += MAP_WG) a.obs_of[i] = -1;
    __syncthreads();
    for (int c = tid; c < n_cams; c += MAP_WG)
        for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++) {
            a.obs_next[m] = -1;
            if (!a.obs_act[m]) continue;
            int *e = a.obs_of + (size_t)c * n_tags + a.obs_tag[m];
            if (*e < 0) { *e = m; continue; }
            int p = *e;
            while (a.obs_next[p] >= 0) p = a.obs_next[p];
            a.obs_next[p] = m;
        }
    __syncthreads();
    // one camera: a pair has one view, every active observation is its pair's first, and no chain is followed (the tag
    // loops below are a few threads walking every camera: a dependent load per entry would double their time)
    const bool chains = a.n_rig > 1;
    auto first = [&](int m) { return a.obs_act[m] && (!chains || a.obs_of[(size_t)a.obs_cam[m] * n_tags + a.obs_tag[m]] == m); };
    auto next = [&](int m) { return chains ? a.obs_next[m] : -1; };
    auto cam_cnt = [&](int c) {
        int k = 0;
        for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++) k += first(m);
        return k;
    };
    map_scan(n_cams, cam_cnt, s_part, a.cam_ptr);
    for (int c = tid; c < n_cams; c += MAP_WG) {
        int o = a.cam_ptr[c];
        for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++)
            if (first(m)) a.cam_obs[o++] = m;
    }
    for (int j = tid; j < n_tags; j += MAP_WG) {
        int k = 0, kp = 0;
        for (int c = 0; c < n_cams; c++) {
            int m = a.obs_of[(size_t)c * n_tags + j];
            kp += m >= 0;
            for (; m >= 0; m = next(m)) k++;
        }
        a.tmp[j] = k;
        a.tmp2[j] = kp;
    }
    __syncthreads();
    const int n_act = map_scan(n_tags, [&](int j) { return a.tmp[j]; }, s_part, a.tag_ptr);
    map_scan(n_tags, [&](int j) { return a.tmp2[j]; }, s_part, a.ptag_ptr);
    for (int j = tid; j < n_tags; j += MAP_WG) {
        int o = a.tag_ptr[j], op = a.ptag_ptr[j];
        for (int c = 0; c < n_cams; c++) {
            int m = a.obs_of[(size_t)c * n_tags + j];
            if (m >= 0) a.ptag_obs[op++] = m;
            for (; m >= 0; m = next(m)) a.tag_obs[o++] = m;
        }
    }
    if (tid == 0) a.head->n_act = n_act;
}

// ---- breadth-first initial map: one workgroup.  A rig: a view's PnP pose is its own camera's, so the frame's pose is
// inv(E_c) T_obs inv(G) and the tag's inv(E_c W) T_obs (LocRig::candidate, camera_pose); the frame half walks the views in
// (camera, slot) order, so a tie of area and tag keeps the lower camera, the tag half in observation order.
template <bool RIG>
__global__ void __launch_bounds__(MAP_WG) k_map_chain(MapArgs a, int n_cams, int n_tags, int n_obs, int wt, double half)
{
    __shared__ int s_changed;
    const int tid = threadIdx.x, S = a.max_tags;
    for (int c = tid; c < n_cams; c += MAP_WG) { a.cam_state[c] = 0; a.cam_seed[c] = -1; pk_eye(a.W + 12 * (size_t)c); }
    for (int j = tid; j < n_tags; j += MAP_WG) { a.tag_state[j] = j == wt; pk_eye(a.G + 12 * (size_t)j); }
    __syncthreads();
    for (;;) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int c = tid; c < n_cams; c += MAP_WG) {
            if (a.cam_state[c]) continue;
            double ba = -1.0;
            int bm = -1, bt = 0x7fffffff;
            for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++) {
                const ObsRec &o = a.obs[a.obs_slot[m]];
                const int j = a.obs_tag[m];
                if (!(o.flags & 2) || !a.tag_state[j]) continue;
                const double ar = loc_area(o.corners);
                if (ar > ba || (ar == ba && j < bt)) { ba = ar; bm = m; bt = j; }
            }
            if (bm < 0) continue;
            double To[12], Gi[12];
            map_obs_pose(a.obs[a.obs_slot[bm]], map_seed_scale(a.tag_half[bt], half), false, To);
            pk_inv(a.G + 12 * (size_t)bt, Gi);
            if constexpr (RIG) {
                double Ei[12], Tc[12];
                pk_inv(map_view_entry(a, bm) + 9, Ei);
                pk_mul(To, Gi, Tc);
                pk_mul(Ei, Tc, a.W + 12 * (size_t)c);
            } else
                pk_mul(To, Gi, a.W + 12 * (size_t)c);
            a.cam_state[c] = 1;
            a.cam_seed[c] = map_view_rig_cam(a, bm) * S + a.obs_slot[bm] % S;  // the frame's global slot
            s_changed = 1;
        }
        __syncthreads();
        for (int j = tid; j < n_tags; j += MAP_WG) {
            if (a.tag_state[j]) continue;
            double ba = -1.0;
            int bm = -1;
            for (int o = a.tag_ptr[j]; o < a.tag_ptr[j + 1]; o++) {  // observation order: a tie keeps the lower camera
                const int m = a.tag_obs[o];
                const ObsRec &r = a.obs[a.obs_slot[m]];
                if (!(r.flags & 2) || !a.cam_state[a.obs_cam[m]]) continue;
                const double ar = loc_area(r.corners);
                if (ar > ba) { ba = ar; bm = m; }
            }
            if (bm < 0) continue;
            double To[12], Wv[12], Wi[12];
            CamDev unused{};
            map_obs_pose(a.obs[a.obs_slot[bm]], map_seed_scale(a.tag_half[j], half), false, To);
            map_view<RIG>(a, unused, bm, a.W + 12 * (size_t)a.obs_cam[bm], unused, Wv);
            pk_inv(Wv, Wi);
            pk_mul(Wi, To, a.G + 12 * (size_t)j);
            a.tag_state[j] = 1;
            s_changed = 1;
        }
        __syncthreads();
        const int ch = s_changed;
        __syncthreads();
        if (!ch) break;
    }
    for (int m = tid; m < n_obs; m += MAP_WG) a.obs_act[m] = a.cam_state[a.obs_cam[m]] == 1 && a.tag_state[a.obs_tag[m]] == 1;
}

// ---- reseed, camera half: one wavefront per camera, k_localize.inc's layout and functions over the frame's slots: one
// camera's max_tags (LocOneCam), or the rig's n_rig * max_tags global slots (LocRig, its table read from a.cams)
template <bool RIG>
__global__ void __launch_bounds__(64) k_map_sweep_cam(MapArgs a, CamDev cam)
{
    extern __shared__ double s_dyn[];
    const int c = blockIdx.x, lane = threadIdx.x, S = RIG ? a.n_rig * a.max_tags : a.max_tags;
    if (a.cam_state[c] != 1) return;
    const LocLds L = loc_lds(s_dyn, S);
    const int f = a.cam_frame[c];
    const LocRig rig{a.cams, a.obs, 65536u / (unsigned int)a.max_tags + 1u, a.n_rig, a.max_tags, a.n_frames, f};
    const LocOneCam one{cam, a.obs + (size_t)f * a.max_tags, a.max_tags};
    auto rec = [&](int s) {
        if constexpr (RIG) return rig.rec(s);
        else return one.rec(s);
    };
    int npart = 0;
    for (int s = lane; s < S; s += ASL_WAVE) {
        const ObsRec *fo = rec(s);
        const int m = a.slot_obs[fo - a.obs];
        const bool part = m >= 0 && a.obs_act[m];
        L.state[s] = part ? 1 : 0;
        L.area[s] = -1.0;
        if (!part) continue;
        npart++;
        double M[12];
        pk_to34(a.G + 12 * (size_t)a.obs_tag[m], M);
        loc_gather_slot(L, s, M, a.tag_half[a.obs_tag[m]], fo->corners);
        if (fo->flags & 2) L.area[s] = loc_area(fo->corners);
    }
    __syncthreads();
    npart = butterfly_sum<64>(npart);
    if (npart == 0) return;
    auto score = [&](const double *P) {
        if constexpr (RIG) return loc_pass<false>(rig, P, P + 9, L, lane, nullptr);
        else return loc_pass<false>(one, P, P + 9, L, lane, nullptr);
    };
    double P[12];
    const double *Wc = a.W + 12 * (size_t)c;
#pragma unroll
    for (int i = 0; i < 12; i++) P[i] = Wc[i];
    double best = score(P);  // the current pose is candidate 0
    int sel[MAP_MAX_CAND];
    const int nsel = loc_top_k(S, lane, [&](int s) { return L.area[s]; }, sel);
    auto make = [&](int s) {
        const ObsRec *fo = rec(s);
        double To[12], M[12];
        const int j = a.obs_tag[a.slot_obs[fo - a.obs]];
        pk_to34(a.G + 12 * (size_t)j, M);
#pragma unroll
        for (int i = 0; i < 12; i++) To[i] = fo->T[i];
        map_scale_obs(To, map_seed_scale(a.tag_half[j], cam.half));
        return [=](bool mirror, double *C) {
            if constexpr (RIG) rig.candidate(s, To, M, mirror, C, C + 9);
            else loc_candidate(To, M, mirror, C, C + 9);
        };
    };
    loc_best_candidate(sel, nsel, make, score, best, P);
    if (lane == 0) {
        double *Wo = a.W + 12 * (size_t)c;
#pragma unroll
        for (int i = 0; i < 12; i++) Wo[i] = P[i];
    }
}

// Total corner cost of world<-tag (R, t), a tag of half side h, over its observations b..e of the active list, the cameras
// held; with NE also the normal equations of the left update of the tag (packed lower triangle 21, then J^T r 6), identical in every lane.
template <bool NE, bool RIG>
__device__ __forceinline__ double map_tag_pass(const MapArgs &a, const CamDev &cam, double h, const double *R, const double *t, int b, int e,
                                               int lane, double *ne)
{
    double cost = 0, acc[27];
#pragma unroll
    for (int i = 0; i < 27; i++) acc[i] = 0;
    for (int k = lane; k < 4 * (e - b); k += ASL_WAVE) {
        const int m = a.tag_obs[b + (k >> 2)], q = k & 3;
        CamDev c;
        double Wc[12];
        map_view<RIG>(a, cam, m, a.W + 12 * (size_t)a.obs_cam[m], c, Wc);
        const ObsRec &o = a.obs[a.obs_slot[m]];
        const double ox = (q == 1 || q == 2) ? h : -h, oy = (q >= 2) ? h : -h;
        double X[3], P[3], uv[2], Jp[6];
#pragma unroll
        for (int r = 0; r < 3; r++) X[r] = R[3 * r] * ox + R[3 * r + 1] * oy + t[r];
#pragma unroll
        for (int r = 0; r < 3; r++) P[r] = Wc[3 * r] * X[0] + Wc[3 * r + 1] * X[1] + Wc[3 * r + 2] * X[2] + Wc[9 + r];
        if (!(P[2] > LOC_Z_MIN)) { cost += LOC_BEHIND_COST; continue; }
        project_dev(c, P, uv, NE ? Jp : nullptr);
        const double r0 = uv[0] - (double)o.corners[2 * q], r1 = uv[1] - (double)o.corners[2 * q + 1];
        if constexpr (NE) {
            double a0[3], a1[3], J0[6], J1[6];  // a = jp R_W: d uv / d X_world
#pragma unroll
            for (int k2 = 0; k2 < 3; k2++) {
                a0[k2] = Jp[0] * Wc[k2] + Jp[1] * Wc[3 + k2] + Jp[2] * Wc[6 + k2];
                a1[k2] = Jp[3] * Wc[k2] + Jp[4] * Wc[3 + k2] + Jp[5] * Wc[6 + k2];
            }
            J0[0] = X[1] * a0[2] - X[2] * a0[1]; J0[1] = X[2] * a0[0] - X[0] * a0[2]; J0[2] = X[0] * a0[1] - X[1] * a0[0];
            J1[0] = X[1] * a1[2] - X[2] * a1[1]; J1[1] = X[2] * a1[0] - X[0] * a1[2]; J1[2] = X[0] * a1[1] - X[1] * a1[0];
#pragma unroll
            for (int k2 = 0; k2 < 3; k2++) { J0[3 + k2] = a0[k2]; J1[3 + k2] = a1[k2]; }
#pragma unroll
            for (int p = 0; p < 6; p++) {
                acc[21 + p] += J0[p] * r0 + J1[p] * r1;
#pragma unroll
                for (int q2 = 0; q2 <= p; q2++) acc[TRI(p, q2)] += J0[p] * J0[q2] + J1[p] * J1[q2];
            }
        }
        cost += r0 * r0 + r1 * r1;
    }
    if constexpr (NE) {
#pragma unroll
        for (int i = 0; i < 27; i++) ne[i] = butterfly_sum<64>(acc[i]);
    }
    return butterfly_sum<64>(cost);
}

// ---- reseed, tag half: one wavefront per tag, the cameras held
template <bool RIG>
__global__ void __launch_bounds__(64) k_map_sweep_tag(MapArgs a, CamDev cam)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    if (a.tag_state[j] != 1) return;
    const int b = a.tag_ptr[j], e = a.tag_ptr[j + 1], n = e - b;
    if (n == 0) return;
    const double h = a.tag_half[j], ks = map_seed_scale(h, cam.half);
    auto score = [&](const double *P) { return map_tag_pass<false, RIG>(a, cam, h, P, P + 9, b, e, lane, nullptr); };
    double P[12];
    const double *Gj = a.G + 12 * (size_t)j;
#pragma unroll
    for (int i = 0; i < 12; i++) P[i] = Gj[i];
    double best = score(P);  // the current pose is candidate 0
    // the <= 8 seeding observations of largest area (ties: lower list position = observation order)
    int sel[MAP_MAX_CAND];
    const int nsel = loc_top_k(n, lane, [&](int o) {
        const ObsRec &rec = a.obs[a.obs_slot[a.tag_obs[b + o]]];
        return (rec.flags & 2) ? loc_area(rec.corners) : -1.0;
    }, sel);
    auto make = [&](int o) {
        const int m = a.tag_obs[b + o];
        double Wv[12], Wi[12];
        CamDev unused;
        map_view<RIG>(a, cam, m, a.W + 12 * (size_t)a.obs_cam[m], unused, Wv);
        pk_inv(Wv, Wi);
        const ObsRec *rec = a.obs + a.obs_slot[m];
        return [=](bool mirror, double *C) {
            double To[12];
            map_obs_pose(*rec, ks, mirror, To);
            pk_mul(Wi, To, C);
        };
    };
    loc_best_candidate(sel, nsel, make, score, best, P);
    if (lane == 0) {
        double *Go = a.G + 12 * (size_t)j;
#pragma unroll
        for (int i = 0; i < 12; i++) Go[i] = P[i];
    }
}

// ---- the gauge: world tag at the identity (one workgroup)
__global__ void __launch_bounds__(MAP_WG) k_map_gauge(MapArgs a, int n_cams, int n_tags, int wt)
{
    __shared__ double sG[12], sGi[12];
    const int tid = threadIdx.x;
    if (tid == 0) {
        for (int i = 0; i < 12; i++) sG[i] = a.G[12 * (size_t)wt + i];
        pk_inv(sG, sGi);
    }
    __syncthreads();
    for (int c = tid; c < n_cams; c += MAP_WG) {
        double Wc[12];
        for (int i = 0; i < 12; i++) Wc[i] = a.W[12 * (size_t)c + i];
        pk_mul(Wc, sG, a.W + 12 * (size_t)c);
    }
    for (int j = tid; j < n_tags; j += MAP_WG) {
        if (j == wt) { pk_eye(a.G + 12 * (size_t)j); continue; }
        double Gj[12];
        for (int i = 0; i < 12; i++) Gj[i] = a.G[12 * (size_t)j + i];
        pk_mul(sGi, Gj, a.G + 12 * (size_t)j);
    }
}

// ---- flip test: one wavefront per tag
template <bool RIG>
__global__ void __launch_bounds__(64) k_map_flip(MapArgs a, CamDev cam, int wt)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j == wt || a.tag_state[j] != 1) return;
    const int b = a.tag_ptr[j], e = a.tag_ptr[j + 1], n = e - b;
    if (n == 0) return;
    const double h = a.tag_half[j];
    double G0[12], R0[9], t0[3], R1[9], t1[3];
    for (int i = 0; i < 12; i++) G0[i] = a.G[12 * (size_t)j + i];
    // the view where the tag is largest (ties: lower list position)
    double ba = -1.0;
    int bo = 0x7fffffff;
    for (int o = lane; o < n; o += ASL_WAVE) {
        const double ar = loc_area(a.obs[a.obs_slot[a.tag_obs[b + o]]].corners);
        if (ar > ba) { ba = ar; bo = o; }
    }
    argmax_step<1>(ba, bo); argmax_step<2>(ba, bo); argmax_step<4>(ba, bo);
    argmax_step<8>(ba, bo); argmax_step<16>(ba, bo); argmax_step<32>(ba, bo);
    double Wb[12];
    {
        const int mb = a.tag_obs[b + bo];
        CamDev unused;
        map_view<RIG>(a, cam, mb, a.W + 12 * (size_t)a.obs_cam[mb], unused, Wb);
    }
    double CT[12], CT34[12], I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, Mr[12], Wi[12], Gm[12];
    pk_mul(Wb, G0, CT);
    pk_to34(CT, CT34);
    loc_candidate(CT34, I34, true, Mr, Mr + 9);
    pk_inv(Wb, Wi);
    pk_mul(Wi, Mr, Gm);
    for (int i = 0; i < 9; i++) { R0[i] = G0[i]; R1[i] = Gm[i]; }
    for (int i = 0; i < 3; i++) { t0[i] = G0[9 + i]; t1[i] = Gm[9 + i]; }
    auto pass = [&](const double *R, const double *t, auto ne_tag, double *ne) {
        return map_tag_pass<decltype(ne_tag)::value, RIG>(a, cam, h, R, t, b, e, lane, ne);
    };
    const double c0 = pose_lm(pass, R0, t0);
    const double c1 = pose_lm(pass, R1, t1);
    if (lane == 0) {
        const bool flip = c1 < c0;
        double *Go = a.G + 12 * (size_t)j;
        for (int i = 0; i < 9; i++) Go[i] = flip ? R1[i] : R0[i];
        for (int i = 0; i < 3; i++) Go[9 + i] = flip ? t1[i] : t0[i];
    }
}

// ---- behind the camera: one thread per camera.  A rig's frame stays with >= 2 distinct tags among its active views.
template <bool RIG>
__global__ void __launch_bounds__(64) k_map_behind(MapArgs a, int n_cams)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cams || a.cam_state[c] != 1) return;
    int k = 0;
    for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++) {
        if (!a.obs_act[m]) continue;
        double Wc[12];
        CamDev unused{};
        map_view<RIG>(a, unused, m, a.W + 12 * (size_t)c, unused, Wc);
        const double *Gj = a.G + 12 * (size_t)a.obs_tag[m];
        const double half = a.tag_half[a.obs_tag[m]];
        bool ok = true;
        for (int q = 0; q < 4; q++) {
            const double ox = (q == 1 || q == 2) ? half : -half, oy = (q >= 2) ? half : -half;
            double X[3];
            for (int r = 0; r < 3; r++) X[r] = Gj[3 * r] * ox + Gj[3 * r + 1] * oy + Gj[9 + r];
            const double z = Wc[6] * X[0] + Wc[7] * X[1] + Wc[8] * X[2] + Wc[11];
            ok = ok && z > MAP_BEHIND_MARGIN;
        }
        a.obs_act[m] = ok;
        if constexpr (RIG)  // an earlier active view of the same tag: counted already
            for (int m2 = a.cam_ptr0[c]; ok && m2 < m; m2++)
                if (a.obs_act[m2] && a.obs_tag[m2] == a.obs_tag[m]) ok = false;
        k += ok;
    }
    if (k < 2) {
        a.cam_state[c] = 3;
        for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++) a.obs_act[m] = 0;
    }
}

__global__ void k_map_lm_init(const MapHead *head, double *lm, double *lm0)
{
    for (int i = 0; i < MAP_LM__N; i++) { lm[i] = 0; lm0[i] = 0; }
    lm[GN_LM_LAMBDA] = 1e-3;
    if (head->n_act == 0) { lm[MAP_LM_STOP] = 1; lm[MAP_LM_STATUS] = 1; }
}

// k_gn_linearize with the k_pnp.inc camera model: one wavefront per observation, gn_obs_block with project_dev; a corner at
// z <= 1e-9 costs 1e12 and adds no row.  Inactive observations cost 0 and leave their block alone (no list refers to it).
// Nothing happens after the stop unless forced.  ROBUST: the Huber loss of threshold hk on the corner's residual length s
// (both components come from the row's one projection): beyond hk the two rows are scaled by sqrt(hk / s) and the corner
// costs 2 hk s - hk^2; a corner's cost is returned once, in its component-0 row.  <false> ignores hk.
// RIG: gn_obs_block gets W = rig<-world, so its p is the rig-frame point; the row applies the view's mounting, projects with
// the view's camera and returns jp = J_proj Re_c, for which the camera block [-[p]x | I] and the tag block are the rig's
// (rig_corner's derivation).
template <bool ROBUST, bool RIG>
__global__ void __launch_bounds__(256) k_map_linearize(MapArgs a, const double *__restrict__ W, const double *__restrict__ G, int n_obs, CamDev cam,
                                                       double *__restrict__ D, double *__restrict__ cost_obs, const double *__restrict__ lm, int force,
                                                       double hk)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n_obs || (!force && lm[MAP_LM_STOP] != 0.0)) return;
    if (!a.obs_act[m]) {
        if (lane == 0) cost_obs[m] = 0.0;
        return;
    }
    const ObsRec &o = a.obs[a.obs_slot[m]];
    auto row = [&](int k, const double *pf, double *jp, double &add) {
        const int comp = k & 1;
        double res = 0;
        jp[0] = 0; jp[1] = 0; jp[2] = 0; add = 0;
        CamDev cv = cam;
        double p[3] = {pf[0], pf[1], pf[2]};
        [[maybe_unused]] const double *Re = nullptr;
        if constexpr (RIG) {
            const double *cl = map_view_entry(a, m), *te = cl + 18;
            Re = cl + 9;
            cv.fx = cl[0]; cv.fy = cl[1]; cv.cx = cl[2]; cv.cy = cl[3]; cv.k1 = cl[4]; cv.k2 = cl[5]; cv.p1 = cl[6]; cv.p2 = cl[7]; cv.k3 = cl[8];
#pragma unroll
            for (int r = 0; r < 3; r++) p[r] = Re[3 * r] * pf[0] + Re[3 * r + 1] * pf[1] + Re[3 * r + 2] * pf[2] + te[r];
        }
        if (p[2] > LOC_Z_MIN) {
            double uv[2], Jp[6];
            project_dev(cv, p, uv, Jp);
            if constexpr (RIG) {  // J_proj Re, both rows
                double Jr[6];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    Jr[r] = Jp[0] * Re[r] + Jp[1] * Re[3 + r] + Jp[2] * Re[6 + r];
                    Jr[3 + r] = Jp[3] * Re[r] + Jp[4] * Re[3 + r] + Jp[5] * Re[6 + r];
                }
#pragma unroll
                for (int r = 0; r < 6; r++) Jp[r] = Jr[r];
            }
            if constexpr (ROBUST) {
                const double r0 = uv[0] - (double)o.corners[k - comp], r1 = uv[1] - (double)o.corners[k - comp + 1];
                const double e = r0 * r0 + r1 * r1, s = sqrt(e);
                const bool over = s > hk;
                const double sw = over ? sqrt(hk / s) : 1.0;
                res = (comp ? r1 : r0) * sw;
#pragma unroll
                for (int r = 0; r < 3; r++) jp[r] = Jp[3 * comp + r] * sw;
                if (comp == 0) add = over ? 2.0 * hk * s - hk * hk : e;
            } else {
                res = uv[comp] - (double)o.corners[k];
#pragma unroll
                for (int r = 0; r < 3; r++) jp[r] = Jp[3 * comp + r];
                add = res * res;
            }
        } else if (comp == 0)
            add = LOC_BEHIND_COST;
        return res;
    };
    const double c = gn_obs_block(W + 12 * (size_t)a.obs_cam[m], G + 12 * (size_t)a.obs_tag[m], a.tag_half[a.obs_tag[m]], lane, row, D + (size_t)m * GN_DSTRIDE);
    if (lane == 0) cost_obs[m] = c;
}

// A rig's pairs with several views: the blocks of the pair's later active views added to its first one's (the one the
// lists and the table hold), in view order; one thread per entry of the block.  Under k_map_linearize's own condition, so
// that a block is folded once per linearisation.
__global__ void __launch_bounds__(256) k_map_fold(MapArgs a, int n_obs, int n_tags, double *__restrict__ D, const double *__restrict__ lm, int force)
{
    const int m = blockIdx.x, e = threadIdx.x;
    if (e >= GN_DSTRIDE || m >= n_obs || (!force && lm[MAP_LM_STOP] != 0.0)) return;
    if (!a.obs_act[m] || a.obs_of[(size_t)a.obs_cam[m] * n_tags + a.obs_tag[m]] != m || a.obs_next[m] < 0) return;
    double acc = D[(size_t)m * GN_DSTRIDE + e];
    for (int m2 = a.obs_next[m]; m2 >= 0; m2 = a.obs_next[m2]) acc += D[(size_t)m2 * GN_DSTRIDE + e];
    D[(size_t)m * GN_DSTRIDE + e] = acc;
}

// The robust call's look at the committed poses (a.W, a.G), one workgroup: wmin_obs[m] = the smallest of observation m's
// four corner weights (0 for an inactive one); sums = {soft observations (a weight < 1), squared error of the corners not
// over hk, their number}, a corner at z <= 1e-9 being one of them with its 1e12.  Per-thread sums in observation order,
// then k_gn_cost's tree.
enum { MAP_SOFT_N = 0, MAP_SOFT_COST, MAP_SOFT_IN, MAP_SOFT__N };
template <bool RIG>
__global__ void __launch_bounds__(256) k_map_soft(MapArgs a, int n_obs, CamDev cam0, double hk, double *__restrict__ wmin_obs, double *__restrict__ sums)
{
    __shared__ double s_cost[256];
    __shared__ int s_soft[256], s_in[256];
    const int tid = threadIdx.x;
    double cost = 0;
    int n_soft = 0, n_in = 0;
    for (int m = tid; m < n_obs; m += 256) {
        double wm = 0.0;
        if (a.obs_act[m]) {
            wm = 1.0;
            const ObsRec &o = a.obs[a.obs_slot[m]];
            const double *Gj = a.G + 12 * (size_t)a.obs_tag[m];
            const double h = a.tag_half[a.obs_tag[m]];
            CamDev cam;
            double Wc[12];
            map_view<RIG>(a, cam0, m, a.W + 12 * (size_t)a.obs_cam[m], cam, Wc);
            for (int q = 0; q < 4; q++) {
                const double ox = (q == 1 || q == 2) ? h : -h, oy = (q >= 2) ? h : -h;
                double X[3], P[3], uv[2];
#pragma unroll
                for (int r = 0; r < 3; r++) X[r] = Gj[3 * r] * ox + Gj[3 * r + 1] * oy + Gj[9 + r];
#pragma unroll
                for (int r = 0; r < 3; r++) P[r] = Wc[3 * r] * X[0] + Wc[3 * r + 1] * X[1] + Wc[3 * r + 2] * X[2] + Wc[9 + r];
                if (!(P[2] > LOC_Z_MIN)) { cost += LOC_BEHIND_COST; n_in++; continue; }
                project_dev(cam, P, uv, nullptr);
                const double r0 = uv[0] - (double)o.corners[2 * q], r1 = uv[1] - (double)o.corners[2 * q + 1];
                const double e = r0 * r0 + r1 * r1, s = sqrt(e);
                if (s > hk) wm = fmin(wm, hk / s);
                else { cost += e; n_in++; }
            }
            n_soft += wm < 1.0;
        }
        wmin_obs[m] = wm;
    }
    s_cost[tid] = cost; s_soft[tid] = n_soft; s_in[tid] = n_in;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) { s_cost[tid] += s_cost[tid + st]; s_soft[tid] += s_soft[tid + st]; s_in[tid] += s_in[tid + st]; }
        __syncthreads();
    }
    if (tid == 0) { sums[MAP_SOFT_N] = s_soft[0]; sums[MAP_SOFT_COST] = s_cost[0]; sums[MAP_SOFT_IN] = s_in[0]; }
}

// accept / reject the trial, count it, stop on a small accepted decrease or a failed factorisation
__global__ void k_map_decide(double *lm, int *fail)
{
    if (lm[MAP_LM_STOP] != 0.0) { lm[GN_LM_FLAG] = 0.0; return; }
    lm[MAP_LM_ITERS] += 1.0;
    if (*fail) { lm[GN_LM_FLAG] = 0.0; lm[MAP_LM_STOP] = 1.0; lm[MAP_LM_STATUS] = 2.0; return; }
    const double cost = lm[GN_LM_COST];
    if (gn_accept(lm) && cost - lm[GN_LM_COST] < 1e-12 * cost) lm[MAP_LM_STOP] = 1.0;
}

// after the stop: the list offsets the LM's k_gn kernels read (a copy) become empty, so that every later trial reduces,
// factors and solves an identity system instead of the real one (its result is discarded anyway)
__global__ void __launch_bounds__(256) k_map_park(const double *__restrict__ lm, int *__restrict__ cam_ptr, int n_cams, int *__restrict__ tag_ptr,
                                                  int n_tags)
{
    if (lm[MAP_LM_STOP] == 0.0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n_cams) cam_ptr[i] = 0;
    else if (i <= n_cams + 1 + n_tags) tag_ptr[i - n_cams - 1] = 0;
}

// Column i of L^-1 by one workgroup of 256: y in LDS (n doubles), forward substitution by blocks of GN_NB with the
// diagonal-block inverses k_gn_chol_diag left in Linv; only the blocks from i's on are touched, so y is zero above row i.
// Returns |L^-1 e_i|^2 in thread 0 (a fixed tree over the threads); y is complete for every thread afterwards.
__device__ __forceinline__ double map_linv_column(const double *__restrict__ S, const double *__restrict__ Linv, int n, int i, double *y)
{
    __shared__ double yb[GN_NB], red[256];
    const int tid = threadIdx.x;
    for (int r = tid; r < n; r += 256) y[r] = r == i ? 1.0 : 0.0;
    __syncthreads();
    const int nblk = (n + GN_NB - 1) / GN_NB;
    for (int bi = i / GN_NB; bi < nblk; bi++) {
        const int k0 = bi * GN_NB, nb = min(GN_NB, n - k0);
        const double *Lb = Linv + (size_t)bi * GN_NB * GN_NB;
        if (tid < nb) {
            double s = 0;
            for (int c = 0; c < nb; c++) s += Lb[tid * GN_NB + c] * y[k0 + c];
            yb[tid] = s;
        }
        __syncthreads();
        if (tid < nb) y[k0 + tid] = yb[tid];
        for (int r = k0 + nb + tid; r < n; r += 256) {
            double s = 0;
            for (int c = 0; c < nb; c++) s += S[(size_t)r * n + k0 + c] * yb[c];
            y[r] -= s;
        }
        __syncthreads();
    }
    double s = 0;
    for (int r = tid; r < n; r += 256) s += y[r] * y[r];
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    return red[0];
}

// diag(S^-1)_i = |L^-1 e_i|^2: one workgroup per tag parameter i
__global__ void __launch_bounds__(256) k_map_std(const double *__restrict__ S, const double *__restrict__ Linv, int n, double *__restrict__ var)
{
    extern __shared__ double y[];
    const double v = map_linv_column(S, Linv, n, blockIdx.x, y);
    if (threadIdx.x == 0) var[blockIdx.x] = v;
}

// ---- the joint covariance of the map (asl_mapcov_*, asl_mapcov_rig_*; tests/map_cov_ref.py): s^2 S^-1 = s^2 Y^T Y with
// Y = L^-1, over the tags k_map_finish numbered (cov_slot: ascending id, neither the world tag nor an unmapped id).
// k_map_cols is k_map_std with the column kept: Yt[i][.] = L^-1 e_i, n doubles, zero before entry i.  The variance is the
// same sum in the same order, so d_tag_std has the bytes of a call without the covariance.
__global__ void __launch_bounds__(256) k_map_cols(const double *__restrict__ S, const double *__restrict__ Linv, int n, double *__restrict__ var,
                                                  double *__restrict__ Yt)
{
    extern __shared__ double y[];
    const int i = blockIdx.x;
    const double v = map_linv_column(S, Linv, n, i, y);
    if (threadIdx.x == 0) var[i] = v;
    for (int r = threadIdx.x; r < n; r += 256) Yt[(size_t)i * n + r] = y[r];
}

// C = s^2 Y^T Y on the matrix pipe: one workgroup per MAP_COV_T x MAP_COV_T tile of the lower triangle, its four
// wavefronts one 16 x 16 block each.  Row p of C is parameter p % 6 of covariance block p / 6, which is row
// 6 cov_tag[p / 6] + p % 6 of Yt.  The K loop runs over the entries of the columns, MAP_COV_KC at a time through LDS
// (A[m][k] = Yt[row p0 + m][k], B[k][n] = Yt[row q0 + n][k], v_mfma_f64_16x16x4_f64 as in k_gn_chol_update), and starts at
// the tile's first row of Yt rounded down to 4: the rows are ascending in p and a column is zero above its own row, so
// everything before that is a product with zero.  The order of every sum depends on the tile alone: the same input gives
// the same bytes.  An entry is computed once, for c <= r, and stored on both sides of the diagonal: symmetric to the bit.
#define MAP_COV_T 32
#define MAP_COV_KC 64
#define MAP_COV_LDP (MAP_COV_KC + 1) /* odd LDS row pitch, as GN_LDP */
__global__ void __launch_bounds__(256) k_map_cov_gram(const double *__restrict__ Yt, int n, const int *__restrict__ cov_tag,
                                                      const int *__restrict__ cov_head, const double *__restrict__ cov_s2,
                                                      double *__restrict__ C, int ld)
{
    const int nc = 6 * cov_head[0];
    const int p0 = blockIdx.x * MAP_COV_T, q0 = blockIdx.y * MAP_COV_T;
    if (blockIdx.y > blockIdx.x || p0 >= nc) return;
    __shared__ double A[MAP_COV_T][MAP_COV_LDP], B[MAP_COV_T][MAP_COV_LDP];
    __shared__ int rowA[MAP_COV_T], rowB[MAP_COV_T];
    const int t = threadIdx.x;
    if (t < MAP_COV_T) {
        const int p = p0 + t, q = q0 + t;
        rowA[t] = p < nc ? 6 * cov_tag[p / 6] + p % 6 : -1;  // past the matrix: a row of zeros
        rowB[t] = q < nc ? 6 * cov_tag[q / 6] + q % 6 : -1;
    }
    __syncthreads();
    const int lane = t & 63, wid = t >> 6, bi = wid >> 1, bj = wid & 1, m = lane & 15, kk = lane >> 4;
    gn_v4d acc = {0, 0, 0, 0};
    for (int k0 = max(rowA[0], rowB[0]) & ~3; k0 < n; k0 += MAP_COV_KC) {
        for (int i = t; i < MAP_COV_T * MAP_COV_KC; i += 256) {
            const int r = i / MAP_COV_KC, c = i - r * MAP_COV_KC, k = k0 + c;
            A[r][c] = (rowA[r] >= 0 && k < n) ? Yt[(size_t)rowA[r] * n + k] : 0.0;
            B[r][c] = (rowB[r] >= 0 && k < n) ? Yt[(size_t)rowB[r] * n + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < MAP_COV_KC / 4; ks++)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[16 * bi + m][4 * ks + kk], B[16 * bj + m][4 * ks + kk], acc, 0, 0, 0);
        __syncthreads();
    }
    const double s2 = *cov_s2;
    // the lane holds rows kk + 4 i of column m of the block
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = p0 + 16 * bi + kk + 4 * i, c = q0 + 16 * bj + m;
        if (r < nc && c < nc && c <= r) {
            const double v = s2 * acc[i];
            C[(size_t)r * ld + c] = v;
            C[(size_t)c * ld + r] = v;
        }
    }
}

// ---- the records: one workgroup.  nothing: no world tag (sizes only, no stage after the gather ran).  wmin_obs and soft
// (k_map_soft's; NULL in a plain call): n_soft, the slot weights and the variance factor over the corners not over the
// threshold; a plain call has n_soft 0, weight 1 for the slots in the solve and cost / dof.  slot_weight may be NULL.
// cov_slot (NULL but in the covariance calls): per id its block of the joint covariance, the ids with a std numbered in
// ascending id, -1 for every other; with it cov_tag[block] = the block's tag, cov_head[0] = the number of blocks and
// *cov_s2 = the variance factor, for k_map_cov_gram.
__global__ void __launch_bounds__(MAP_WG) k_map_finish(MapArgs a, int n_cams, int n_tags, int n_obs, int wt, int nothing, const double *lm,
                                                       const double *cost_obs, const double *seed_obs, const double *var, const int *var_fail,
                                                       const double *wmin_obs, const double *soft, MapTagRec *map,
                                                       double *tag_std, CamPoseRec *poses, MapResultRec *res, double *slot_weight,
                                                       int *cov_slot, int *cov_tag, int *cov_head, double *cov_s2)
{
    __shared__ int s_part[MAP_WG + 1];
    const int tid = threadIdx.x;
    const int n_act = nothing ? 0 : map_scan(n_obs, [&](int m) { return a.obs_act[m]; }, s_part, nullptr);
    const int n_used = nothing ? 0 : map_scan(n_cams, [&](int c) { return a.cam_state[c] == 1 ? 1 : 0; }, s_part, nullptr);
    auto mapped = [&](int j) { return j == wt || a.tag_ptr[j + 1] > a.tag_ptr[j]; };
    const int n_mapped = nothing ? 0 : map_scan(n_tags, [&](int j) { return (a.tag_state[j] == 1 && mapped(j)) ? 1 : 0; }, s_part, nullptr);
    int status = nothing ? 1 : (int)lm[MAP_LM_STATUS];
    const double cost = nothing ? 0.0 : lm[GN_LM_COST], cost0 = nothing ? 0.0 : lm[GN_LM_COST0];
    if (status == 0 && !isfinite(cost)) status = 3;
    const int dof = 8 * n_act - 6 * n_used - 6 * (n_mapped - 1);
    double s2 = dof > 0 ? cost / dof : 0.0;
    if (soft) {
        const int dof_in = 2 * (int)soft[MAP_SOFT_IN] - 6 * n_used - 6 * (n_mapped - 1);
        s2 = dof_in > 0 ? soft[MAP_SOFT_COST] / dof_in : 0.0;
    }
    const bool std_ok = var && !(var_fail && *var_fail);  // an undamped system that is not positive definite gives no std
    for (int f = tid; f < a.n_frames; f += MAP_WG) {
        CamPoseRec *o = poses + f;
        const int np = a.fr_npart[f];
        const bool used = a.fr_ndist[f] >= 2;
        int st = 1, na = 0, seed = -1;
        double T[12], rms = 0, rms0 = 0;
        pk_eye(T);
        if (used) {
            const int c = a.fr_cam[f];
            st = nothing ? 5 : (a.cam_state[c] == 1 ? (status == 0 ? 0 : 4) : a.cam_state[c] == 3 ? 3 : 5);
            seed = nothing ? -1 : a.cam_seed[c];
            if (st == 0 || st == 4) {
                double e = 0, e0 = 0;
                for (int m = a.cam_ptr0[c]; m < a.cam_ptr0[c + 1]; m++)
                    if (a.obs_act[m]) { na++; e += cost_obs[m]; e0 += seed_obs[m]; }
                pk_inv(a.W + 12 * (size_t)c, T);
                if (na) { rms = sqrt(e / (4.0 * na)); rms0 = sqrt(e0 / (4.0 * na)); }
            }
        }
        for (int r = 0; r < 3; r++) {
            o->T[4 * r] = T[3 * r]; o->T[4 * r + 1] = T[3 * r + 1]; o->T[4 * r + 2] = T[3 * r + 2]; o->T[4 * r + 3] = T[9 + r];
        }
        o->T[12] = 0; o->T[13] = 0; o->T[14] = 0; o->T[15] = 1;
        o->rms_px = rms; o->rms_seed_px = rms0;
        o->n_tags = na;
        o->n_rejected = used ? np - na : 0;
        o->status = st;
        o->seed_slot = seed;
    }
    for (int i = tid; i < a.n_ids; i += MAP_WG) {
        const int j = (!nothing && a.seen[i]) ? a.id_tag[i] : -1;
        const bool ok = j >= 0 && status == 0 && a.tag_state[j] == 1 && mapped(j);
        MapTagRec *r = map + i;
        double T[12];
        if (ok) pk_to34(a.G + 12 * (size_t)j, T);
        for (int k = 0; k < 12; k++) r->T[k] = ok ? T[k] : 0.0;
        r->valid = ok ? 1 : 0;
        r->size = ok ? a.sizes[i] : 0.0f;
        if (tag_std)
            for (int k = 0; k < 6; k++) tag_std[6 * (size_t)i + k] = (ok && j != wt && std_ok) ? sqrt(s2 * var[6 * j + k]) : 0.0;
    }
    if (cov_slot) {
        auto has = [&](int i) {
            const int j = (!nothing && a.seen[i]) ? a.id_tag[i] : -1;
            return (j >= 0 && status == 0 && a.tag_state[j] == 1 && mapped(j) && j != wt && std_ok) ? 1 : 0;
        };
        const int n_cov = map_scan(a.n_ids, has, s_part, a.tmp);
        for (int i = tid; i < a.n_ids; i += MAP_WG) {
            const bool h = has(i);
            cov_slot[i] = h ? a.tmp[i] : -1;
            if (h) cov_tag[a.tmp[i]] = a.id_tag[i];
        }
        if (tid == 0) { cov_head[0] = n_cov; *cov_s2 = s2; }
    }
    if (slot_weight)
        for (size_t k = tid; k < (size_t)a.n_rig * a.n_frames * a.max_tags; k += MAP_WG) {
            const int m = nothing ? -1 : a.slot_obs[k];
            slot_weight[k] = (m >= 0 && status == 0 && a.obs_act[m]) ? (wmin_obs ? wmin_obs[m] : 1.0) : 0.0;
        }
    if (tid == 0) {
        MapResultRec r;
        r.cost_seed = cost0; r.cost = cost;
        r.rms_px = n_act ? sqrt(cost / (4.0 * n_act)) : 0.0;
        r.rms_seed_px = n_act ? sqrt(cost0 / (4.0 * n_act)) : 0.0;
        r.n_frames_used = status == 0 ? n_used : 0;
        r.n_tags = status == 0 ? n_mapped : 0;
        r.n_obs = n_act;
        r.n_obs_dropped = n_obs - n_act;
        r.iterations = nothing ? 0 : (int)lm[MAP_LM_ITERS];
        r.world_id = a.head->world_id;
        r.status = status;
        r.n_soft = (soft && status == 0) ? (int)soft[MAP_SOFT_N] : 0;
        *res = r;
    }
}
