// Sequence localisation against a fixed tag map with a random-walk motion prior (asl_smooth_frames_device /
// asl_smooth_batch): one camera<-world pose per frame of one camera's consecutive frames, minimising the reprojection
// error of all mapped corners (/ sigma_px^2) plus |(Log(R_D) / sigma_rot, t_D / sigma_trans)|^2 between consecutive
// frames, R_D = R_{f+1} R_f^T, t_D = t_{f+1} - R_D t_f.  tests/smooth_ref.py is the NumPy statement of the same
// computation, operation order of the linear solve included.  float64, contraction off, no scratch.  One frame step is one
// unit of time unless the call gives the frames' times (below).
// asl_smooth_robust_sequences_* (huber_px > 0): the same launches with k_smooth_cand<true> and k_smooth_lin<true>, which put every
// corner's pixel residual through a Huber loss (loc_corner<NE, true>, k_localize.inc): its cost in every place the squared
// one stands, its weight on J^T J and J^T r, and per frame the number of slots with a corner over the threshold, carried
// with the state (SmoothSet.soft) as the pixel cost is.  tests/smooth_ref.py states it at huber_px > 0.  The plain calls run
// the <false> instantiations: the code they ran before, the counts 0.
// asl_smooth_timed_sequences_* (SmoothBufs.times, n doubles on the device): frame f is at time times[f], and sigma_rot and
// sigma_trans are the random walk's per unit of that time.  The pair (f, f + 1) of a sequence, dt = times[f + 1] - times[f], has
// m_f = (Log(R_D) w_rot, t_D w_trans), w_rot = (1 / sigma_rot) (1 / sqrt(dt)), w_trans = (1 / sigma_trans) (1 / sqrt(dt)), in
// that operation order, so dt == 1 is the plain weight to the bit; k_smooth_lin's Jacobians, blocks and |m|^2 are built from
// them, and the solve, the decide and the covariance read those blocks as they are.  The chain divides a transition cost by
// times[f] - times[p] where the plain call divides by f - p.  Times of two sequences are unrelated.  A sequence with a time that
// is not finite or a dt <= 0 is found by k_smooth_scan and solved as one without a posed frame, result status 4.  Every other
// call leaves times NULL: a branch on the pointer, one value in the whole launch, ahead of each of the three places; no
// instantiation of its own.  tests/smooth_ref.py states it (times).
// asl_smooth_rig_sequences_* (a rig, k_rig.inc): the pose solved for is rig<-world, a frame's slots are the n_cams * max_tags
// global slots of the camera-major block.  Only the two kernels that cost corners look at a camera, and their bodies are
// written once over a slot model (smooth_cand_frame, smooth_lin_frame; loc_solve_frame does the same for the localisation):
// k_smooth_cand / k_smooth_lin are set-up, LocOneCam and one call, k_smooth_rig_cand / k_smooth_rig_lin the camera table to
// LDS, LocRig and the same call.  Every other kernel below runs as it is.  tests/smooth_ref.py states it (smooth_rig).
//   seed chain   k_smooth_cand   one wavefront per frame: the seed's pose A and, for a frame of exactly one taking-part slot,
//                                its mirrored planar minimum B (loc_candidate), both costed over the frame's corners
//                k_smooth_scan   one wavefront a sequence: the nearest posed frame at or before every frame (wave_scan of a maximum)
//                k_smooth_trans  one thread per posed frame: the four motion costs from its predecessor's candidates
//                k_smooth_dp     one wavefront a sequence: the two-state dynamic programme, forward and back, 64 frames' costs a load
//                k_smooth_fill   one thread per frame: the chosen pose, or the nearest earlier posed frame's
//                k_smooth_lin    (below) once at the chain's poses, then k_smooth_init: one workgroup a sequence, the cost after the
//                                chain, the LM state (lambda0, status 1 / 3), the per-frame seed costs
//   per trial    k_smooth_lin    one wavefront per frame: the pose (stepped by delta), the frame's cost, H and g from its
//                                corners (loc_gather, loc_pass), and the motion blocks of the pair (f, f + 1), a lane an entry
//                k_smooth_solve  one wavefront a sequence: the block-tridiagonal Cholesky forward and back over the frames, the 6x6
//                                block spread over 36 lanes with its operands in LDS (forward step: smooth_chol6, smooth_couple)
//                k_smooth_decide one workgroup a sequence: the trial's cost in a fixed order (smooth_sums), the accept rule, lambda, the stop
//                k_smooth_commit the accepted trials copied over the current state (smooth_set_at), spread over the device
//   end          k_smooth_finish one thread per frame: the records (n_rejected: the frame's soft slots; n_soft: lm[SM_SOFT], their
//                                sum over the sequence by k_smooth_init / k_smooth_decide's fixed-order sums)
//   covariance   k_smooth_cov    (asl_smooth_cov_*, only when asked for) one wavefront a sequence: the undamped block Cholesky of the
//                                returned state forward (the solve's forward step under its own pivot rule), the diagonal blocks of
//                                the inverse back, a 6x6 block from frame to frame
//                k_smooth_cov_finish  one thread per frame: sigma_px, dof, status, and the zeros of a status 1 / 2
// Several sequences per call (asl_smooth_sequences_*): sequence k is the frames [seq[k], seq[k + 1]) of the call's, with its own
// lm[SM__N] and head[SMH__N]; no term links two sequences.  The chain kernels and the per-sequence sums run one workgroup per
// sequence, each over its own frames with the arithmetic of the single-sequence call, indexed from the sequence's first
// frame; a per-frame kernel reads the state of its frame's sequence (smooth_seq_of).  The single-sequence calls are n_seq = 1:
// the same launches, the one range {0, n} taken from the arguments (smooth_seq), no table.
// Serial by nature are the scan, the dynamic programme and the factor-and-solve: each is a chain over the frames, so each
// is one wavefront that carries a small state (a maximum, two costs, a 6x6 coupling block) from frame to frame.  All trials are enqueued at once;
// lm[SM_STOP] makes the ones after the stop return at once (k_map.inc works the same way).

struct SmoothResultRec {  // == asl_smooth_result, 64 bytes
    double cost_seed, cost, rms_px, rms_seed_px;
    int32_t n_frames_data, n_filled, n_flipped, iterations, status, n_soft, reserved[2];
};

enum { SM_COST = 0, SM_LAMBDA, SM_STOP, SM_ITERS, SM_STATUS, SM_COST0, SM_SOLVED, SM_PIX, SM_PIX0, SM_CORNERS, SM_NDATA, SM_TAKE, SM_COV, SM_SOFT, SM__N = 16 };
enum { SMH_NPOSED = 0, SMH_FIRST, SMH_FAIL, SMH_NFLIP, SMH_BADT, SMH__N = 8 };   // SMH_BADT: the sequence's times are bad (status 4)
#define SM_MOT 121                // per pair: QN 36, QP 36, C 36, gN 6, gP 6, |m|^2
// One state's arrays, in doubles per frame from the start of the allocation: pose (R 9, t 3), packed normal equations
// (21 + 6), pixel cost, soft slots, motion blocks.  smooth_set() and smooth_set_at() are the two readings of this layout.
enum { SMS_POSE = 0, SMS_NE = 12, SMS_PIX = 39, SMS_SOFT = 40, SMS_MOT = 41 };
#define SM_SET (SMS_MOT + SM_MOT)  // doubles per frame of one state
#define SM_FAC 84                 // per frame of the factorisation: L 36, M 36, 1 / diag 6, y 6 (k_smooth_cov: the undamped one, no y)
#define SM_WG 256

// One state of the solve over n frames, one allocation (soft slots: the robust call's, 0 from the plain ones; motion blocks:
// of the pairs (f, f + 1))
struct SmoothSet {
    double *P, *ne, *c, *soft, *mot;
};

__host__ __device__ inline SmoothSet smooth_set(double *base, size_t n)
{
    return {base + SMS_POSE * n, base + SMS_NE * n, base + SMS_PIX * n, base + SMS_SOFT * n, base + SMS_MOT * n};
}

// Entry e (0 <= e < SM_SET) of frame f in a state of n frames: the index from the allocation's start
__host__ __device__ inline size_t smooth_set_at(int e, size_t f, size_t n)
{
    if (e < SMS_NE) return SMS_POSE * n + (SMS_NE - SMS_POSE) * f + (e - SMS_POSE);
    if (e < SMS_PIX) return SMS_NE * n + (SMS_PIX - SMS_NE) * f + (e - SMS_NE);
    if (e < SMS_MOT) return (size_t)e * n + f;   // pixel cost, soft slots: one double a frame each
    return SMS_MOT * n + SM_MOT * f + (e - SMS_MOT);
}

struct SmoothBufs {
    double *cand, *dcost, *tcost;   // per frame: A and B (2 x 12), their weighted data costs (2), transitions (4: from * 2 + to)
    int *posed, *ntags, *src, *back, *choice, *code, *head;
    double *lm, *cseed, *delta, *fac;
    double *set[2];                 // the current state and the trial
    int *seq, *fseq;                // n_seq > 1: the sequences' first frames (n_seq + 1) and every frame's sequence (k_smooth_seqs)
    const double *times;            // the timed calls' frame times (n); NULL: frame f is at time f
    int n, n_seq;                   // lm and head: n_seq of each
};

// Sequence k of a call: frames [f0, f0 + n)
struct SmoothSeq {
    int k, f0, n;
};

__device__ __forceinline__ SmoothSeq smooth_seq(const SmoothBufs &b, int k)
{
    if (b.n_seq == 1) return {0, 0, b.n};
    const int f0 = b.seq[k];
    return {k, f0, b.seq[k + 1] - f0};
}

// The same for a k that is one value in the whole wavefront (a workgroup a sequence): the range in scalar registers, so
// that the loops over the frames and their addresses stay scalar, as they are with the one range of the arguments
__device__ __forceinline__ SmoothSeq smooth_seq_uniform(const SmoothBufs &b, int k)
{
    const SmoothSeq q = smooth_seq(b, k);
    return {__builtin_amdgcn_readfirstlane(q.k), __builtin_amdgcn_readfirstlane(q.f0), __builtin_amdgcn_readfirstlane(q.n)};
}

// The sequence of frame f
__device__ __forceinline__ SmoothSeq smooth_seq_of(const SmoothBufs &b, int f)
{
    return smooth_seq(b, b.n_seq == 1 ? 0 : b.fseq[f]);
}

// The same for an f that is one value in the whole wavefront (a wavefront or a workgroup a frame)
__device__ __forceinline__ SmoothSeq smooth_seq_of_uniform(const SmoothBufs &b, int f)
{
    return smooth_seq_uniform(b, b.n_seq == 1 ? 0 : b.fseq[f]);
}

// The offsets of up to SM_SEQ_CHUNK sequences, carried in the launch's own arguments: they reach the device in stream order
// without a staging buffer that a later call could overwrite, and the host array is free when the launch returns.
#define SM_SEQ_CHUNK 896
struct SmoothSeqChunk {
    int k0, count;                  // sequences [k0, k0 + count)
    int32_t start[SM_SEQ_CHUNK + 1];
};

// One workgroup per sequence of the chunk: its entry of seq (the last one also the end) and its frames' entries of fseq
__global__ void __launch_bounds__(SM_WG) k_smooth_seqs(SmoothBufs b, SmoothSeqChunk c)
{
    const int j = (int)blockIdx.x, k = c.k0 + j, f0 = c.start[j], f1 = c.start[j + 1];
    if (threadIdx.x == 0) {
        b.seq[k] = f0;
        if (j + 1 == c.count) b.seq[k + 1] = f1;
    }
    for (int f = f0 + (int)threadIdx.x; f < f1; f += SM_WG) b.fseq[f] = k;
}

__device__ __forceinline__ void smooth_relative(const double *Ra, const double *ta, const double *Rb, const double *tb, double *RD, double *tD)
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) RD[3 * i + j] = Rb[3 * i] * Ra[3 * j] + Rb[3 * i + 1] * Ra[3 * j + 1] + Rb[3 * i + 2] * Ra[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; i++) tD[i] = tb[i] - (RD[3 * i] * ta[0] + RD[3 * i + 1] * ta[1] + RD[3 * i + 2] * ta[2]);
}

// m = (Log(R_D) isr, t_D ist) of the poses a = (R_f, t_f) and b = (R_{f+1}, t_{f+1}); returns |m|^2
__device__ __forceinline__ double smooth_residual(const double *Pa, const double *Pb, double isr, double ist, double *RD, double *tD, double *m)
{
    smooth_relative(Pa, Pa + 9, Pb, Pb + 9, RD, tD);
    const double a[3] = {0.5 * (RD[7] - RD[5]), 0.5 * (RD[2] - RD[6]), 0.5 * (RD[3] - RD[1])};
    const double s = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double c = 0.5 * ((RD[0] + RD[4] + RD[8]) - 1.0);
    const double k = s > 1e-12 ? atan2(s, c) / s : 1.0;
    double mm = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) m[i] = (s > 1e-12 ? a[i] * k : a[i]) * isr;
#pragma unroll
    for (int i = 0; i < 3; i++) m[3 + i] = tD[i] * ist;
#pragma unroll
    for (int i = 0; i < 6; i++) mm += m[i] * m[i];
    return mm;
}

// P <- [Rod(w) | v] P, d = (w, v): the localisation's left update
__device__ __forceinline__ void smooth_update(double *P, const double *d)
{
    double dR[9], Rn[9], tn[3];
    rodrigues_dev(d, dR);
    mat3_mul_dev(dR, P, Rn);
#pragma unroll
    for (int r = 0; r < 3; r++) tn[r] = dR[3 * r] * P[9] + dR[3 * r + 1] * P[10] + dR[3 * r + 2] * P[11] + d[3 + r];
#pragma unroll
    for (int i = 0; i < 9; i++) P[i] = Rn[i];
    P[9] = tn[0]; P[10] = tn[1]; P[11] = tn[2];
}

// [t]x (a, b), t in LDS (indexed at run time: not a register array)
__device__ __forceinline__ double smooth_skew(const double *t, int a, int b)
{
    if (a == b) return 0.0;
    const double v = t[3 - a - b];
    return (b - a + 3) % 3 == 1 ? -v : v;
}

// sum over the workgroup (SM_WG threads) in a fixed order, in every thread; sh: SM_WG doubles
__device__ __forceinline__ double smooth_block_sum(double v, double *sh)
{
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = SM_WG / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// A sequence's sums over a state, each in smooth_block_sum's fixed order and in every thread: the cost (pixel costs w + the
// pairs' |m|^2), the pixel cost, the soft slots.  frame(f, c): what else the caller does with frame f and its pixel cost c.
struct SmoothSums {
    double cost, pix, soft;
};

template <class Frame>
__device__ __forceinline__ SmoothSums smooth_sums(const SmoothSet &s, const SmoothSeq &q, double w, double *sh, Frame frame)
{
    double cost = 0, pix = 0, soft = 0;
    for (int lf = (int)threadIdx.x; lf < q.n; lf += SM_WG) {
        const int f = q.f0 + lf;
        const double c = s.c[f];
        frame(f, c);
        soft += s.soft[f];
        cost += c * w + (lf + 1 < q.n ? s.mot[SM_MOT * (size_t)f + 120] : 0.0);
        pix += c;
    }
    cost = smooth_block_sum(cost, sh);
    pix = smooth_block_sum(pix, sh);
    soft = smooth_block_sum(soft, sh);
    return {cost, pix, soft};
}

// Candidates of frame f and their data costs over the slots of model m, by one wavefront; ROBUST: under the Huber loss of
// threshold hk pixels (the model's corner), as every later cost of the call is.  Written once for k_smooth_cand (LocOneCam)
// and k_smooth_rig_cand (LocRig), as loc_solve_frame is for the localisation.  Pose A is the seed's body<-world (the
// camera's, or the rig's).  B, for a frame of exactly one taking-part slot over the whole model: that slot's camera<-tag =
// (camera<-world of its camera at A) map[id], mirrored and taken back through inv(map[id]) and the model's candidate().
template <bool ROBUST, class Model>
__device__ __forceinline__ void smooth_cand_frame(const Model &m, const LocLds &L, const MapTagRec *__restrict__ map, int n_ids, double half,
                                                  const CamPoseRec *__restrict__ seed, double w, const SmoothBufs &b, double hk, int f, int lane)
{
    const int n = m.nslots();
    const int npart = loc_gather([&](int s) { return m.rec(s); }, n, map, n_ids, half, [](int) { return false; }, L, lane);
    const bool posed = seed[f].status == 0;
    if (lane == 0) { b.ntags[f] = npart; b.posed[f] = posed ? 1 : 0; }
    if (!posed) return;
    double RA[9], tA[3], RB[9], tB[3];
    const double *T = seed[f].T;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) RA[3 * i + j] = T[4 * j + i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) tA[i] = -(RA[3 * i] * T[3] + RA[3 * i + 1] * T[7] + RA[3 * i + 2] * T[11]);
    [[maybe_unused]] int soft;
    const auto data_cost = [&](const double *R, const double *t) {
        if constexpr (ROBUST) return loc_pass<false, true>(m, R, t, L, lane, nullptr, hk, &soft);
        else return loc_pass<false>(m, R, t, L, lane, nullptr);
    };
    const double dA = data_cost(RA, tA) * w;
    double dB = dA;
    const bool has_b = npart == 1;
    if (has_b) {  // the one taking-part slot: the only term of the sum
        int ls = 0;
        for (int s = lane; s < n; s += ASL_WAVE)
            if (L.state[s] == 1) ls += s;
        const int s1 = butterfly_sum<64>(ls);
        const double *Mp = map[m.rec(s1)->id].T;
        double M[12], To[12], Rc[9], tc[3];
#pragma unroll
        for (int k = 0; k < 12; k++) M[k] = Mp[k];
        m.camera_pose(s1, RA, tA, Rc, tc);
#pragma unroll
        for (int i = 0; i < 3; i++) {  // camera<-tag = (camera<-world) map[id]
#pragma unroll
            for (int j = 0; j < 4; j++)
                To[4 * i + j] = Rc[3 * i] * M[j] + Rc[3 * i + 1] * M[4 + j] + Rc[3 * i + 2] * M[8 + j] + (j == 3 ? tc[i] : 0.0);
        }
        m.candidate(s1, To, M, true, RB, tB);
        dB = data_cost(RB, tB) * w;
    }
    if (lane == 0) {
        double *c = b.cand + 24 * (size_t)f;
#pragma unroll
        for (int i = 0; i < 9; i++) { c[i] = RA[i]; c[12 + i] = has_b ? RB[i] : RA[i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { c[9 + i] = tA[i]; c[21 + i] = has_b ? tB[i] : tA[i]; }
        b.dcost[2 * f] = dA;
        b.dcost[2 * f + 1] = dB;
    }
}

// One camera: one wavefront per frame, the frame's max_tags records
template <bool ROBUST>
__global__ void __launch_bounds__(64) k_smooth_cand(const ObsRec *__restrict__ obs, int max_tags, const MapTagRec *__restrict__ map, int n_ids,
                                                    CamDev cam, const CamPoseRec *__restrict__ seed, double w, SmoothBufs b, double hk)
{
    extern __shared__ double s_dyn[];
    const int f = (int)blockIdx.x;
    const LocOneCam m{cam, obs + (size_t)f * max_tags, max_tags};
    smooth_cand_frame<ROBUST>(m, loc_lds(s_dyn, max_tags), map, n_ids, cam.half, seed, w, b, hk, f, (int)threadIdx.x);
}

// A rig (asl_smooth_rig_sequences_*): one wavefront per frame over its n_cams * max_tags global slots in the camera-major
// block obs[n_cams][n_frames][max_tags], n_frames the frames of the whole call; the camera table to LDS first, as
// k_localize_rig fills it; dynamic LDS rig_lds_bytes(n_cams, max_tags).  seed and the poses solved for are the rig's.
template <bool ROBUST>
__global__ void __launch_bounds__(64) k_smooth_rig_cand(const ObsRec *__restrict__ obs, int n_cams, int n_frames, int max_tags,
                                                        const MapTagRec *__restrict__ map, int n_ids, const RigCamRec *__restrict__ rig, double half,
                                                        const CamPoseRec *__restrict__ seed, double w, SmoothBufs b, double hk)
{
    extern __shared__ double s_dyn[];
    const int lane = (int)threadIdx.x, f = (int)blockIdx.x;
    rig_fill_cams(s_dyn, rig, n_cams, lane);
    const LocRig m{s_dyn, obs, 65536u / (unsigned int)max_tags + 1u, n_cams, max_tags, n_frames, f};
    smooth_cand_frame<ROBUST>(m, loc_lds(s_dyn + RIG_CAM_DOUBLES * n_cams, m.nslots()), map, n_ids, half, seed, w, b, hk, f, lane);
}

// A sequence's src[f]: the nearest posed frame of the sequence at or before f (-1: none), as a frame of the call; its head:
// the number of posed frames and the first one.  Timed: a time that is not finite, or a pair of the sequence with
// times[f + 1] - times[f] <= 0, makes it a sequence without a posed frame and sets SMH_BADT (k_smooth_init: status 4)
__global__ void __launch_bounds__(64) k_smooth_scan(SmoothBufs b)
{
    const int lane = (int)threadIdx.x;
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    int *head = b.head + SMH__N * q.k;
    int carry = -1, np = 0, first = -1, bad = 0;
    for (int base = 0; base < q.n; base += ASL_WAVE) {
        const int f = q.f0 + base + lane;
        const bool in = base + lane < q.n;
        if (b.times && in) {  // one value in the whole wavefront: the plain calls skip it
            const double t = b.times[f];
            bad |= !isfinite(t) || (base + lane > 0 && !(t - b.times[f - 1] > 0)) ? 1 : 0;
        }
        const int v = (in && b.posed[f]) ? f : -1;
        int s = wave_scan<false>(v, -1, [](int x, int y) { return x > y ? x : y; });
        s = s > carry ? s : carry;
        if (in) b.src[f] = s;
        carry = readlane(s, 63);
        np += butterfly_sum<64>(v >= 0 ? 1 : 0);
        const int mn = wave_scan<true>(v >= 0 ? v : 0x7fffffff, 0x7fffffff, [](int x, int y) { return x < y ? x : y; });
        if (first < 0 && mn != 0x7fffffff) first = mn;
    }
    bad = butterfly_sum<64>(bad) != 0;
    if (bad) np = 0;   // nothing is solved: every kernel after this one treats the sequence as one without a posed frame
    if (lane == 0) { head[SMH_NPOSED] = np; head[SMH_FIRST] = first; head[SMH_FAIL] = 0; head[SMH_NFLIP] = 0; head[SMH_BADT] = bad; }
}

// The four transition costs of a posed frame from its predecessor, over a gap of g frame steps (timed: of g = times[f] -
// times[p]) divided by g
__global__ void __launch_bounds__(64) k_smooth_trans(SmoothBufs b, double isr, double ist)
{
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f >= b.n || !b.posed[f]) return;
    const int p = f > smooth_seq_of(b, f).f0 ? b.src[f - 1] : -1;
    double *tc = b.tcost + 4 * (size_t)f;
    if (p < 0) { tc[0] = 0; tc[1] = 0; tc[2] = 0; tc[3] = 0; return; }
    const double gap = b.times ? b.times[f] - b.times[p] : (double)(f - p);
    double Pa[12], Pb[12], RD[9], tD[3], m[6];
    for (int a = 0; a < 2; a++)
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int k = 0; k < 12; k++) { Pa[k] = b.cand[24 * (size_t)p + 12 * a + k]; Pb[k] = b.cand[24 * (size_t)f + 12 * c + k]; }
            tc[2 * a + c] = smooth_residual(Pa, Pb, isr, ist, RD, tD, m) / gap;
        }
}

// The dynamic programme over the posed frames: forward (ties to A), then back from the lower-cost state (tie: A).  A lane
// loads one frame of each chunk of 64; the chain reads them lane by lane (readlane) and leaves lane l's result with lane l.
__global__ void __launch_bounds__(64) k_smooth_dp(SmoothBufs b)
{
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    int *head = b.head + SMH__N * q.k;
    if (head[SMH_NPOSED] == 0) return;
    const int lane = (int)threadIdx.x, n = q.n;
    double cA = 0, cB = 0;
    bool started = false;
    for (int base = 0; base < n; base += ASL_WAVE) {
        const int f = q.f0 + base + lane;
        const bool in = base + lane < n;
        const int my = (in && b.posed[f]) ? 1 : 0;
        double dA = 0, dB = 0, t00 = 0, t01 = 0, t10 = 0, t11 = 0;
        if (my) {
            dA = b.dcost[2 * f]; dB = b.dcost[2 * f + 1];
            t00 = b.tcost[4 * (size_t)f]; t01 = b.tcost[4 * (size_t)f + 1]; t10 = b.tcost[4 * (size_t)f + 2]; t11 = b.tcost[4 * (size_t)f + 3];
        }
        int my_back = 0;
        for (int l = 0; l < ASL_WAVE; l++) {
            if (!readlane(my, l)) continue;
            const double a = readlane(dA, l), bb = readlane(dB, l);
            int bk = 0;
            if (!started) {
                cA = a; cB = bb; started = true;
            } else {
                double best = cA + readlane(t00, l), alt = cB + readlane(t10, l);
                if (alt < best) { best = alt; bk |= 1; }
                const double nA = best + a;
                best = cA + readlane(t01, l); alt = cB + readlane(t11, l);
                if (alt < best) { best = alt; bk |= 2; }
                cB = best + bb;
                cA = nA;
            }
            if (lane == l) my_back = bk;
        }
        if (in) b.back[f] = my_back;   // read back below by the lane that wrote it
    }
    int cur = cB < cA ? 1 : 0, nflip = 0;
    for (int base = (n - 1) / ASL_WAVE * ASL_WAVE; base >= 0; base -= ASL_WAVE) {
        const int f = q.f0 + base + lane;
        const bool in = base + lane < n;
        const int my = (in && b.posed[f]) ? 1 : 0;
        const int my_back = in ? b.back[f] : 0;
        int my_choice = 0;
        for (int l = ASL_WAVE - 1; l >= 0; l--) {
            if (!readlane(my, l)) continue;
            if (lane == l) my_choice = cur;
            nflip += cur;
            cur = (readlane(my_back, l) >> cur) & 1;
        }
        if (in) b.choice[f] = my_choice;
    }
    if (lane == 0) head[SMH_NFLIP] = nflip;
}

// Every frame's start pose and seed code; the soft-slot counts of both states start at 0 (the robust k_smooth_lin alone
// writes them again)
__global__ void __launch_bounds__(SM_WG) k_smooth_fill(SmoothBufs b, const CamPoseRec *__restrict__ seed)
{
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f >= b.n) return;
    smooth_set(b.set[0], (size_t)b.n).soft[f] = 0.0;
    smooth_set(b.set[1], (size_t)b.n).soft[f] = 0.0;
    const int *head = b.head + SMH__N * smooth_seq_of(b, f).k;
    if (head[SMH_NPOSED] == 0) return;
    int s = b.src[f];
    if (s < 0) s = head[SMH_FIRST];
    const int ch = b.choice[s];
    const double *c = b.cand + 24 * (size_t)s + 12 * ch;
    double *P = b.set[0] + 12 * (size_t)f;
    for (int k = 0; k < 12; k++) P[k] = c[k];
    b.code[f] = b.posed[f] ? seed[f].seed_slot + LOC_MIRRORED * ch : -1;
}

// Frame f of a state: its pose (trial: the current one stepped by delta), pixel cost, H and g, and the motion blocks of
// the pair (f, f + 1) at the same state.  ROBUST: the cost is the Huber loss of threshold hk pixels, H and g are the sums
// weighted by it (iteratively reweighted Gauss-Newton, no second-order term), and the state carries the frame's soft slots.
// Timed: the pair's weights are (isr, ist) / sqrt(times[f + 1] - times[f]), the random walk's over that time.
// The body is written once over a slot model, as smooth_cand_frame is: smooth_lin_runs says whether the frame's wavefront
// has work (before any set-up), smooth_lin_frame does it; SmoothLinLds is the kernel's static LDS.
struct SmoothLinLds {
    double RD[9], tD[3], m[6], B[36], Ad[36], Jn[36], Jp[36];
};

__device__ __forceinline__ bool smooth_lin_runs(const SmoothBufs &b, int f, int trial, SmoothSeq &q)
{
    q = smooth_seq_of_uniform(b, f);
    const int *head = b.head + SMH__N * q.k;
    if (head[SMH_NPOSED] == 0) return false;
    if (trial && (b.lm[SM__N * q.k + SM_STOP] != 0.0 || head[SMH_FAIL])) return false;
    return true;
}

template <bool ROBUST, class Model>
__device__ __forceinline__ void smooth_lin_frame(const Model &m, const LocLds &L, SmoothLinLds &sh, const MapTagRec *__restrict__ map, int n_ids,
                                                 double half, const SmoothBufs &b, const SmoothSeq &q, int trial, double isr, double ist, double hk,
                                                 int f, int lane)
{
    const int n = b.n;
    const SmoothSet in = smooth_set(b.set[0], (size_t)n), out = smooth_set(b.set[trial], (size_t)n);
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; k++) P[k] = in.P[12 * (size_t)f + k];
    if (trial) {
        double d[6];
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = b.delta[6 * (size_t)f + k];
        smooth_update(P, d);
    }
    loc_gather([&](int s) { return m.rec(s); }, m.nslots(), map, n_ids, half, [](int) { return false; }, L, lane);
    double ne[27], c;
    [[maybe_unused]] int soft;
    if constexpr (ROBUST) c = loc_pass<true, true>(m, P, P + 9, L, lane, ne, hk, &soft);
    else c = loc_pass<true>(m, P, P + 9, L, lane, ne);
    if (lane == 0) {
        if (trial) {  // trial 0 linearises the current state in place: its poses stay as they are (block f - 1 reads them)
#pragma unroll
            for (int k = 0; k < 12; k++) out.P[12 * (size_t)f + k] = P[k];
        }
#pragma unroll
        for (int k = 0; k < 27; k++) out.ne[27 * (size_t)f + k] = ne[k];
        out.c[f] = c;
        if constexpr (ROBUST) out.soft[f] = (double)soft;   // the plain kernel leaves k_smooth_fill's 0
    }
    if (f + 1 >= q.f0 + q.n) return;   // the last frame of its sequence: no pair

    double Q[12], RD[9], tD[3], mv[6];
#pragma unroll
    for (int k = 0; k < 12; k++) Q[k] = in.P[12 * (size_t)(f + 1) + k];
    if (trial) {
        double d[6];
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = b.delta[6 * (size_t)(f + 1) + k];
        smooth_update(Q, d);
    }
    if (b.times) {  // one value in the whole wavefront; a step of exactly 1 leaves both weights as they are
        const double isd = 1.0 / sqrt(b.times[f + 1] - b.times[f]);
        isr = isr * isd;
        ist = ist * isd;
    }
    const double mm = smooth_residual(P, Q, isr, ist, RD, tD, mv);
    double *mot = out.mot + SM_MOT * (size_t)f;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) sh.RD[k] = RD[k];
#pragma unroll
        for (int k = 0; k < 3; k++) sh.tD[k] = tD[k];
#pragma unroll
        for (int k = 0; k < 6; k++) sh.m[k] = mv[k];
        mot[120] = mm;
    }
    __syncthreads();
    const int i = lane / 6, j = lane % 6;   // lanes 0..35: entry (i, j) of a 6x6 block
    if (lane < 36) {  // B = [[I, 0], [-[t_D]x, I]], Ad = [[R_D, 0], [[t_D]x R_D, R_D]]
        double bv = i == j ? 1.0 : 0.0, av = 0.0;
        if (i >= 3 && j < 3) {
            bv = -smooth_skew(sh.tD, i - 3, j);
            av = smooth_skew(sh.tD, i - 3, 0) * sh.RD[j] + smooth_skew(sh.tD, i - 3, 1) * sh.RD[3 + j] + smooth_skew(sh.tD, i - 3, 2) * sh.RD[6 + j];
        } else if (i < 3 && j < 3)
            av = sh.RD[3 * i + j];
        else if (i >= 3 && j >= 3)
            av = sh.RD[3 * (i - 3) + j - 3];
        sh.B[lane] = bv;
        sh.Ad[lane] = av;
    }
    __syncthreads();
    if (lane < 36) {  // Jn = W B, Jp = -W B Ad
        const double wi = i < 3 ? isr : ist;
        double s = 0;
        for (int k = 0; k < 6; k++) s += sh.B[6 * i + k] * sh.Ad[6 * k + j];
        sh.Jn[lane] = wi * sh.B[lane];
        sh.Jp[lane] = -(wi * s);
    }
    __syncthreads();
    if (lane < 36) {
        double qn = 0, qp = 0, cc = 0;
        for (int k = 0; k < 6; k++) {
            qn += sh.Jp[6 * k + i] * sh.Jp[6 * k + j];
            qp += sh.Jn[6 * k + i] * sh.Jn[6 * k + j];
            cc += sh.Jn[6 * k + i] * sh.Jp[6 * k + j];
        }
        mot[lane] = qn;
        mot[36 + lane] = qp;
        mot[72 + lane] = cc;
    }
    if (lane < 6) {
        double gn = 0, gp = 0;
        for (int k = 0; k < 6; k++) { gn += sh.Jp[6 * k + lane] * sh.m[k]; gp += sh.Jn[6 * k + lane] * sh.m[k]; }
        mot[108 + lane] = gn;
        mot[114 + lane] = gp;
    }
}

template <bool ROBUST>
__global__ void __launch_bounds__(64) k_smooth_lin(const ObsRec *__restrict__ obs, int max_tags, const MapTagRec *__restrict__ map, int n_ids,
                                                   CamDev cam, SmoothBufs b, int trial, double isr, double ist, double hk)
{
    extern __shared__ double s_dyn[];
    __shared__ SmoothLinLds s_lin;
    const int f = (int)blockIdx.x;
    SmoothSeq q;
    if (!smooth_lin_runs(b, f, trial, q)) return;
    const LocOneCam m{cam, obs + (size_t)f * max_tags, max_tags};
    smooth_lin_frame<ROBUST>(m, loc_lds(s_dyn, max_tags), s_lin, map, n_ids, cam.half, b, q, trial, isr, ist, hk, f, (int)threadIdx.x);
}

// The rig's, set up as k_smooth_rig_cand
template <bool ROBUST>
__global__ void __launch_bounds__(64) k_smooth_rig_lin(const ObsRec *__restrict__ obs, int n_cams, int n_frames, int max_tags,
                                                       const MapTagRec *__restrict__ map, int n_ids, const RigCamRec *__restrict__ rig, double half,
                                                       SmoothBufs b, int trial, double isr, double ist, double hk)
{
    extern __shared__ double s_dyn[];
    __shared__ SmoothLinLds s_lin;
    const int lane = (int)threadIdx.x, f = (int)blockIdx.x;
    SmoothSeq q;
    if (!smooth_lin_runs(b, f, trial, q)) return;
    rig_fill_cams(s_dyn, rig, n_cams, lane);
    const LocRig m{s_dyn, obs, 65536u / (unsigned int)max_tags + 1u, n_cams, max_tags, n_frames, f};
    smooth_lin_frame<ROBUST>(m, loc_lds(s_dyn + RIG_CAM_DOUBLES * n_cams, m.nslots()), s_lin, map, n_ids, half, b, q, trial, isr, ist, hk, f, lane);
}

// After the chain's linearisation: the LM state, the seed costs
__global__ void __launch_bounds__(SM_WG) k_smooth_init(SmoothBufs b, double w)
{
    __shared__ double sh[SM_WG];
    const int tid = (int)threadIdx.x;
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    double *lm = b.lm + SM__N * q.k;
    if (b.head[SMH__N * q.k + SMH_NPOSED] == 0) {
        if (tid < SM__N) lm[tid] = 0.0;
        __syncthreads();
        if (tid == 0) { lm[SM_STOP] = 1.0; lm[SM_STATUS] = b.head[SMH__N * q.k + SMH_BADT] ? 4.0 : 1.0; }
        return;
    }
    const SmoothSet s = smooth_set(b.set[0], (size_t)b.n);
    double corners = 0, ndata = 0;
    const SmoothSums sum = smooth_sums(s, q, w, sh, [&](int f, double c) {
        b.cseed[f] = c;
        corners += 4.0 * b.ntags[f];
        ndata += b.ntags[f] > 0 ? 1.0 : 0.0;
    });
    const double cost = sum.cost, pix = sum.pix, soft = sum.soft;
    corners = smooth_block_sum(corners, sh);
    ndata = smooth_block_sum(ndata, sh);
    if (tid == 0) {
        const bool bad = !isfinite(cost);
        lm[SM_COST] = cost; lm[SM_COST0] = cost; lm[SM_PIX] = pix; lm[SM_PIX0] = pix; lm[SM_CORNERS] = corners; lm[SM_NDATA] = ndata;
        lm[SM_SOFT] = soft;
        lm[SM_LAMBDA] = 1e-3; lm[SM_ITERS] = 0.0; lm[SM_SOLVED] = 0.0;
        lm[SM_STOP] = bad ? 1.0 : 0.0;
        lm[SM_STATUS] = bad ? 3.0 : 0.0;
    }
}

// The forward step both k_smooth_solve and k_smooth_cov take at a frame, S = S_f in LDS, lane 6 i + j its entry (i, j).
// smooth_chol6: the right-looking Cholesky of S in place (every entry loses its products in the order k = 0, 1, ..., as
// chol6_solve_tri_dev's do), 1 / diagonal in inv in every lane.  pivot(p, c): whether pivot p of column c passes; returns
// whether all six did, the same LDS words in every lane, so one value in the whole wavefront.  No exit at a failed pivot:
// the columns after it work on a spoilt block, which the caller, who then writes its flag and leaves, never reads.
template <class Pivot>
__device__ __forceinline__ bool smooth_chol6(double *S, int lane, int i, int j, double *inv, Pivot pivot)
{
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double p = S[7 * c];
        ok &= pivot(p, c);
        const double dc = sqrt(p);
        inv[c] = 1.0 / dc;
        __syncthreads();
        if (lane < 36 && j == c) {
            if (i == c) S[lane] = dc;
            else if (i > c) S[lane] = S[lane] * inv[c];
        }
        __syncthreads();
        if (lane < 36 && j > c && i >= j) S[lane] = S[lane] - S[6 * i + c] * S[6 * j + c];
        __syncthreads();
    }
    return ok;
}

// smooth_couple: row `lane` of M_f = C_f L_f^-T from the factored S (pair: frame f has a successor; C: C_f, row-major),
// then L, 1 / diag, M (and the solve's y, if any) into the frame's fac and M_f into Mp for the next frame: every load
// ahead of the first store
__device__ __forceinline__ void smooth_couple(const double *S, const double *inv, const double *y, const double *C, bool pair, int lane, int i,
                                              int j, double *Mp, double *fac)
{
    double Mr[6] = {0, 0, 0, 0, 0, 0};
    if (pair && lane < 6) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double t = C[6 * lane + c];
#pragma unroll
            for (int k = 0; k < c; k++) t -= Mr[k] * S[6 * c + k];
            Mr[c] = t * inv[c];
        }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 6; a++) {
            fac[72 + a] = inv[a];
            if (y) fac[78 + a] = y[a];
        }
    }
    if (lane < 36) fac[lane] = i >= j ? S[lane] : 0.0;
    if (pair && lane < 6) {
#pragma unroll
        for (int c = 0; c < 6; c++) { Mp[6 * lane + c] = Mr[c]; fac[36 + 6 * lane + c] = Mr[c]; }
    }
    __syncthreads();
}

// (A + lambda diag(A)) delta = -g, A block tridiagonal: forward S_f = A_ff (damped) - M_{f-1} M_{f-1}^T = L_f L_f^T,
// L_f y_f = -g_f - M_{f-1} y_{f-1}, M_f = C_f L_f^-T; back L_f^T x_f = y_f - M_f^T x_{f+1}.  Lane 6 i + j holds entry (i, j)
// of the block on its way through smooth_chol6; the triangular solves of six numbers run in every lane on the same LDS
// operands.  A pivot that is not positive sets head[SMH_FAIL] and ends the kernel.
__global__ void __launch_bounds__(64) k_smooth_solve(SmoothBufs b, double w)
{
    __shared__ double S[36], Mp[36], yv[6], rr[6], iv[6];
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    const double *lm = b.lm + SM__N * q.k;
    if (lm[SM_STOP] != 0.0) return;
    const int lane = (int)threadIdx.x, n = q.n, i = lane / 6, j = lane % 6;
    const double lambda = lm[SM_LAMBDA];
    const SmoothSet s = smooth_set(b.set[0], (size_t)b.n);
    // from here on at the sequence's first frame: f counts from it, and the addresses advance by constants
    const double *nes = s.ne + 27 * (size_t)q.f0, *mots = s.mot + SM_MOT * (size_t)q.f0;
    double *facs = b.fac + SM_FAC * (size_t)q.f0, *delta = b.delta + 6 * (size_t)q.f0;
    for (int f = 0; f < n; f++) {
        const double *ne = nes + 27 * (size_t)f, *mot = mots + SM_MOT * (size_t)f, *motp = mot - SM_MOT;
        double v = 0;
        if (lane < 36) {
            v = ne[i >= j ? TRI(i, j) : TRI(j, i)] * w;
            if (f > 0) v = v + motp[36 + lane];
            if (f + 1 < n) v = v + mot[lane];
            if (i == j) v = v + lambda * v;
            if (f > 0)
                for (int k = 0; k < 6; k++) v = v - Mp[6 * i + k] * Mp[6 * j + k];
        } else if (lane < 42) {
            const int r = lane - 36;
            double g = ne[21 + r] * w;
            if (f > 0) g = g + motp[114 + r];
            if (f + 1 < n) g = g + mot[108 + r];
            v = -g;
            if (f > 0)
                for (int k = 0; k < 6; k++) v = v - Mp[6 * r + k] * yv[k];
        }
        __syncthreads();
        if (lane < 36) S[lane] = v;
        else if (lane < 42) rr[lane - 36] = v;
        __syncthreads();
        double inv[6];
        if (!smooth_chol6(S, lane, i, j, inv, [](double p, int) { return p > 0; })) {
            if (lane == 0) b.head[SMH__N * q.k + SMH_FAIL] = 1;
            return;
        }
        double y[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double t = rr[a];
#pragma unroll
            for (int k = 0; k < a; k++) t -= S[6 * a + k] * y[k];
            y[a] = t * inv[a];
        }
        if (lane == 0) {  // read again only at the top of the next frame, after smooth_couple's barriers
#pragma unroll
            for (int a = 0; a < 6; a++) yv[a] = y[a];
        }
        smooth_couple(S, inv, y, mot + 72, f + 1 < n, lane, i, j, Mp, facs + SM_FAC * (size_t)f);
    }
    __threadfence();  // fac: written by some lanes, read by others below
    double x[6] = {0, 0, 0, 0, 0, 0};
    for (int f = n - 1; f >= 0; f--) {
        const double *fac = facs + SM_FAC * (size_t)f;   // written above by this wavefront
        __syncthreads();
        if (lane < 36) { S[lane] = fac[lane]; Mp[lane] = f + 1 < n ? fac[36 + lane] : 0.0; }
        if (lane < 6) { iv[lane] = fac[72 + lane]; yv[lane] = fac[78 + lane]; }
        __syncthreads();
        double r[6], xn[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double t = yv[a];
            if (f + 1 < n) {
#pragma unroll
                for (int k = 0; k < 6; k++) t -= Mp[6 * k + a] * x[k];
            }
            r[a] = t;
        }
#pragma unroll
        for (int a = 5; a >= 0; a--) {
            double t = r[a];
#pragma unroll
            for (int k = a + 1; k < 6; k++) t -= S[6 * k + a] * xn[k];
            xn[a] = t * iv[a];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) x[a] = xn[a];
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 6; a++) delta[6 * (size_t)f + a] = x[a];
        }
    }
}

// The trial's cost and the localisation's accept rule on it; lm[SM_TAKE]: k_smooth_commit has a trial to copy
__global__ void __launch_bounds__(SM_WG) k_smooth_decide(SmoothBufs b, double w)
{
    __shared__ double sh[SM_WG];
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    double *lm = b.lm + SM__N * q.k;
    int *head = b.head + SMH__N * q.k;
    const int tid = (int)threadIdx.x;
    if (lm[SM_STOP] != 0.0) {
        if (tid == 0) lm[SM_TAKE] = 0.0;
        return;
    }
    const bool failed = head[SMH_FAIL] != 0;
    const double cost = lm[SM_COST];
    __syncthreads();
    if (failed) {
        if (tid == 0) { lm[SM_ITERS] += 1.0; lm[SM_LAMBDA] *= 10.0; lm[SM_TAKE] = 0.0; head[SMH_FAIL] = 0; }
        return;
    }
    const SmoothSums sum = smooth_sums(smooth_set(b.set[1], (size_t)b.n), q, w, sh, [](int, double) {});
    const double cn = sum.cost, pix = sum.pix, soft = sum.soft;
    const bool take = cn < cost;
    if (tid == 0) {
        lm[SM_ITERS] += 1.0;
        lm[SM_SOLVED] = 1.0;
        lm[SM_TAKE] = take ? 1.0 : 0.0;
        if (take) {
            if (cost - cn < 1e-12 * cost) lm[SM_STOP] = 1.0;
            lm[SM_COST] = cn;
            lm[SM_PIX] = pix;
            lm[SM_SOFT] = soft;
            lm[SM_LAMBDA] *= 0.1;
        } else
            lm[SM_LAMBDA] *= 10.0;
    }
}

// A workgroup a frame at a time, where the frame's sequence took its trial: a thread an entry of the frame's SM_SET (pose,
// normal equations, pixel cost, soft slots, the pair's motion blocks)
__global__ void __launch_bounds__(SM_WG) k_smooth_commit(SmoothBufs b)
{
    if (b.n_seq == 1 && b.lm[SM_TAKE] == 0.0) return;
    const size_t n = (size_t)b.n;
    const int e = (int)threadIdx.x;
    for (size_t f = blockIdx.x; f < n; f += gridDim.x) {
        if (e >= SM_SET || b.lm[SM__N * smooth_seq_of_uniform(b, (int)f).k + SM_TAKE] == 0.0) continue;
        const size_t at = smooth_set_at(e, f, n);
        b.set[0][at] = b.set[1][at];
    }
}

__global__ void __launch_bounds__(SM_WG) k_smooth_finish(SmoothBufs b, CamPoseRec *__restrict__ out, SmoothResultRec *__restrict__ res)
{
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x), n = b.n;
    if (f >= n) return;
    const SmoothSeq q = smooth_seq_of(b, f);
    const double *lm = b.lm + SM__N * q.k;
    const int *head = b.head + SMH__N * q.k;
    const bool nothing = head[SMH_NPOSED] == 0;
    int status = (int)lm[SM_STATUS];
    if (!nothing && status == 0 && lm[SM_SOLVED] == 0.0) status = 2;
    if (f == q.f0) {
        res += q.k;
        const double k = nothing ? 0.0 : lm[SM_CORNERS];
        res->cost_seed = nothing ? 0.0 : lm[SM_COST0];
        res->cost = nothing ? 0.0 : lm[SM_COST];
        res->rms_px = k > 0 ? sqrt(lm[SM_PIX] / k) : 0.0;
        res->rms_seed_px = k > 0 ? sqrt(lm[SM_PIX0] / k) : 0.0;
        res->n_frames_data = nothing ? 0 : (int)lm[SM_NDATA];
        res->n_filled = nothing ? 0 : q.n - head[SMH_NPOSED];
        res->n_flipped = nothing ? 0 : head[SMH_NFLIP];
        res->iterations = (int)lm[SM_ITERS];
        res->status = status;
        res->n_soft = nothing ? 0 : (int)lm[SM_SOFT];
        res->reserved[0] = 0; res->reserved[1] = 0;
    }
    CamPoseRec *o = out + f;
    if (nothing) { loc_write_none(o, 1); return; }
    const SmoothSet s = smooth_set(b.set[0], (size_t)n);
    const double *R = s.P + 12 * (size_t)f, *t = R + 9;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        o->T[4 * r] = R[r]; o->T[4 * r + 1] = R[3 + r]; o->T[4 * r + 2] = R[6 + r];
        o->T[4 * r + 3] = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
    }
    o->T[12] = 0; o->T[13] = 0; o->T[14] = 0; o->T[15] = 1;
    const int nt = b.ntags[f];
    o->rms_px = nt > 0 ? sqrt(s.c[f] / (4.0 * nt)) : 0.0;
    o->rms_seed_px = nt > 0 ? sqrt(b.cseed[f] / (4.0 * nt)) : 0.0;
    o->n_tags = nt;
    o->n_rejected = (int)s.soft[f];
    o->status = status != 0 ? 4 : nt > 0 ? 0 : 6;
    o->seed_slot = b.code[f];
}

// The covariance of the returned poses (asl_smooth_cov_*): the diagonal blocks of A^-1, A the undamped matrix of
// k_smooth_solve at set[0] (the state k_smooth_finish writes out; its blocks are the ones linearised there).  Forward as the
// solve's, lambda = 0: S_f = D_f - M_{f-1} M_{f-1}^T = L_f L_f^T, M_f = C_f L_f^-T, kept in b.fac (free once the trials are
// over; the LM's own last factor is damped and may be a rejected trial's).  Back, Sigma_{f+1} carried in LDS:
//   Sigma_f = L_f^-T (I + M_f^T Sigma_{f+1} M_f) L_f^-1
// T = Sigma_{f+1} M_f and X = I + M_f^T T an entry a lane (lane 6 i + j: entry (i, j)), then L^T Z = X a column a lane and
// L^T Y^T = Z^T a row a lane.  Y's lower triangle, mirrored, is Sigma_f: the carry and, as R^T . R on each 3x3 block
// (world<-camera: A = diag(-R^T, -R^T), the sign drops out), lower triangle mirrored again, the record's cov.
// lm[SM_COV] is the status of every record: 1 without a solve, 2 if a pivot p of column c of S_f is not above
// max(0, POSE_COV_PIVOT_TOL D_f[c][c]) (the inverse is global: no frame has a covariance then), else 0.  A lane loads the
// next frame's operands before it works on the current one: the chain waits for arithmetic, not for memory.
__global__ void __launch_bounds__(64) k_smooth_cov(SmoothBufs b, double w, PoseCovRec *__restrict__ cov)
{
    __shared__ double S[36], Mp[36], Cs[36], Sg[36], T[36], X[36], Rm[9], iv[6], dg[6];
    const SmoothSeq q = smooth_seq_uniform(b, (int)blockIdx.x);
    const int lane = (int)threadIdx.x, n = q.n, i = lane / 6, j = lane % 6;
    double *lm = b.lm + SM__N * q.k;
    if (b.head[SMH__N * q.k + SMH_NPOSED] == 0 || lm[SM_STATUS] != 0.0 || lm[SM_SOLVED] == 0.0) {
        if (lane == 0) lm[SM_COV] = 1.0;
        return;
    }
    SmoothSet s = smooth_set(b.set[0], (size_t)b.n);   // from here on at the sequence's first frame: f counts from it
    s.P += 12 * (size_t)q.f0; s.ne += 27 * (size_t)q.f0; s.mot += SM_MOT * (size_t)q.f0;
    double *facs = b.fac + SM_FAC * (size_t)q.f0;
    cov += q.f0;
    const int tri = i >= j ? TRI(i, j) : TRI(j, i);
    double h = 0, qn = 0, cc = 0, qp = 0;   // frame f's H, QN_f, C_f and QP_{f-1} entry of this lane
    if (lane < 36) {
        h = s.ne[tri];
        if (n > 1) { qn = s.mot[lane]; cc = s.mot[72 + lane]; }
    }
#pragma clang loop unroll(disable)   // nor peeled: one copy of the frame's body, not a second one for f = 0
    for (int f = 0; f < n; f++) {
        double v = 0;
        if (lane < 36) {
            v = h * w;
            if (f > 0) v = v + qp;
            if (f + 1 < n) v = v + qn;
        }
        const double d = v, c0 = cc;
        qp = 0;
        if (lane < 36 && f + 1 < n) {  // the next frame's
            const double *mot = s.mot + SM_MOT * (size_t)f;
            qp = mot[36 + lane];
            h = s.ne[27 * (size_t)(f + 1) + tri];
            if (f + 2 < n) { qn = mot[SM_MOT + lane]; cc = mot[SM_MOT + 72 + lane]; }
        }
        if (lane < 36 && f > 0)
            for (int k = 0; k < 6; k++) v = v - Mp[6 * i + k] * Mp[6 * j + k];
        __syncthreads();
        if (lane < 36) {
            S[lane] = v;
            Cs[lane] = c0;
            if (i == j) dg[i] = d;
        }
        __syncthreads();
        double inv[6];
        if (!smooth_chol6(S, lane, i, j, inv, [&](double p, int c) { return p > 0 && p > POSE_COV_PIVOT_TOL * dg[c]; })) {
            if (lane == 0) lm[SM_COV] = 2.0;
            return;
        }
        smooth_couple(S, inv, nullptr, Cs, f + 1 < n, lane, i, j, Mp, facs + SM_FAC * (size_t)f);
    }
    __threadfence();  // fac: written by some lanes, read by others below
    if (lane == 0) lm[SM_COV] = 0.0;
    double l = 0, m = 0, iq = 0, r = 0;   // frame f's L, M, 1 / diag and R entry of this lane
    {
        const double *fac = facs + SM_FAC * (size_t)(n - 1);
        if (lane < 36) l = fac[lane];
        if (lane < 6) iq = fac[72 + lane];
        if (lane < 9) r = s.P[12 * (size_t)(n - 1) + lane];
    }
    for (int f = n - 1; f >= 0; f--) {
        __syncthreads();
        if (lane < 36) { S[lane] = l; Mp[lane] = m; }
        if (lane < 6) iv[lane] = iq;
        if (lane < 9) Rm[lane] = r;
        if (f > 0) {  // the next frame's
            const double *fac = facs - SM_FAC + SM_FAC * (size_t)f;
            if (lane < 36) { l = fac[lane]; m = fac[36 + lane]; }
            if (lane < 6) iq = fac[72 + lane];
            if (lane < 9) r = s.P[12 * (size_t)(f - 1) + lane];
        }
        __syncthreads();
        double x = i == j ? 1.0 : 0.0;
        if (f + 1 < n) {
            if (lane < 36) {
                double t = 0;
                for (int k = 0; k < 6; k++) t += Sg[6 * i + k] * Mp[6 * k + j];
                T[lane] = t;
            }
            __syncthreads();
            if (lane < 36) {
                double a = 0;
                for (int k = 0; k < 6; k++) a += Mp[6 * k + i] * T[6 * k + j];
                x = x + a;
            }
        }
        if (lane < 36) X[lane] = x;
        __syncthreads();
        if (lane < 6) {  // column `lane` of Z = L^-T X
            double z[6];
#pragma unroll
            for (int a = 5; a >= 0; a--) {
                double t = X[6 * a + lane];
#pragma unroll
                for (int k = a + 1; k < 6; k++) t -= S[6 * k + a] * z[k];
                z[a] = t * iv[a];
            }
#pragma unroll
            for (int a = 0; a < 6; a++) T[6 * a + lane] = z[a];
        }
        __syncthreads();
        if (lane < 6) {  // row `lane` of Y = Z L^-1
            double y[6];
#pragma unroll
            for (int a = 5; a >= 0; a--) {
                double t = T[6 * lane + a];
#pragma unroll
                for (int k = a + 1; k < 6; k++) t -= S[6 * k + a] * y[k];
                y[a] = t * iv[a];
            }
#pragma unroll
            for (int a = 0; a < 6; a++) X[6 * lane + a] = y[a];
        }
        __syncthreads();
        if (lane < 36) Sg[lane] = X[i >= j ? lane : 6 * j + i];
        __syncthreads();
        if (lane < 36) {  // U = Sigma diag(R, R)
            const int c0 = 6 * i + 3 * (j / 3), jj = j % 3;
            T[lane] = Sg[c0] * Rm[jj] + Sg[c0 + 1] * Rm[3 + jj] + Sg[c0 + 2] * Rm[6 + jj];
        }
        __syncthreads();
        if (lane < 36) {  // diag(R, R)^T U
            const int r0 = 18 * (i / 3) + j, ii = i % 3;
            X[lane] = Rm[ii] * T[r0] + Rm[3 + ii] * T[r0 + 6] + Rm[6 + ii] * T[r0 + 12];
        }
        __syncthreads();
        if (lane < 36) cov[f].cov[lane] = X[i >= j ? lane : 6 * j + i];
    }
}

// What every record of the sequence shares, and the zeros of a sequence without a covariance
__global__ void __launch_bounds__(SM_WG) k_smooth_cov_finish(SmoothBufs b, double sigma_px, PoseCovRec *__restrict__ cov)
{
    const int f = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (f >= b.n) return;
    const double *lm = b.lm + SM__N * smooth_seq_of(b, f).k;
    const int status = (int)lm[SM_COV];
    PoseCovRec *o = cov + f;
    if (status != 0) {
#pragma unroll
        for (int k = 0; k < 36; k++) o->cov[k] = 0.0;
    }
    o->sigma_px = sigma_px;
    o->dof = status == 1 ? 0 : 2 * (int)lm[SM_CORNERS] - 6;   // 8 a taking-part slot, less the 6 of one free pose
    o->status = status;
}
