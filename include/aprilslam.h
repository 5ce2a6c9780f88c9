/*
 * include/aprilslam.h -- C ABI of libaprilslam.so, the MI355X (gfx950) AprilTag-SLAM hot path.
 *
 * Drop-in boundary.  The reference reaches its hot path through two native packages:
 *   apriltag(tag_type).detect(gray)                 reference src/detection/tag_detector.py:11,18,26
 *   cv2.cvtColor(image, cv2.COLOR_BGR2GRAY)         reference src/detection/tag_detector.py:25
 *   cv2.solvePnP(obj_points, corners, K, dist)      reference src/detection/tag_detector.py:41
 *   cv2.Rodrigues(rvec)                             reference src/detection/tag_detector.py:47
 * Upstream's `apriltag` module is a CPython extension, so there is no existing FFI
 * signature to copy; the entry points below are what a ctypes binding for that module
 *  needs.  Plain pointers and sizes only; no torch / HIP types.
 *
 * Conventions
 *   - every function returns 0 on success and a negative ASL_E* code on failure;
 *     asl_last_error() returns a thread-local message for the last failure.
 *   - "host" pointers are ordinary process memory, "device" pointers are HIP device
 *     memory on the detector's GPU (e.g. torch.Tensor.data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - images are row-major uint8, `stride` = bytes between rows, 1 channel (gray) or
 *     3 channels (BGR, as cv2 hands them to TagDetector.detect).
 *   - pixel convention: pixel (ix, iy) covers [ix, ix+1) x [iy, iy+1), centre at +0.5.
 *   - one detector per (host thread, stream); a detector is not re-entrant
 *     (same rule as upstream's detector object).
 *   - there is NO CPU fallback: without a usable gfx950 device every call fails.
 */
#ifndef APRILSLAM_H
#define APRILSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASL_OK 0
#define ASL_EINVAL (-1)      /* bad argument (unknown family, unsupported decimate/blur, NULL pointer ...) */
#define ASL_EDEVICE (-2)     /* HIP runtime / no GPU */
#define ASL_ECAPACITY (-3)   /* an internal work buffer overflowed even after growing */
#define ASL_ENOMEM (-4)

typedef struct asl_detector asl_detector;

/* One detection: the fields of the dict upstream's wrapper returns
   ('id', 'hamming', 'margin', 'center', 'lb-rb-rt-lt'), plus the frame index inside a batch. */
typedef struct {
    int32_t id;
    int32_t hamming;
    float margin;
    int32_t frame;
    double center[2];
    double corners[4][2]; /* lb, rb, rt, lt in pixels (reference tag_detector.py:32) */
} asl_detection;

/* Pose of one detection: what TagDetector.get_pose returns (reference tag_detector.py:30-43). */
typedef struct {
    double rvec[3];
    double tvec[3];
    double T[16]; /* row-major camera<-tag 4x4 (reference tag_detector.py:45-52) */
    int32_t ok;   /* solvePnP's retval */
    int32_t reserved;
} asl_pose;

/* Replaces `apriltag(family, threads=1, maxhamming=1, decimate=2.0, blur=0.0, refine_edges=True)`
   (reference tag_detector.py:18 passes the family only; the wrapper's defaults apply).
   decimate must be an integer value >= 1 (the reference never sets it).  blur must be 0 here: upstream's blur
   (quad_sigma) is set on the created detector with asl_detector_set_quad_sigma.
   device = HIP device ordinal. */
int asl_detector_create(const char *family, int nthreads, int maxhamming, float decimate, float blur,
                        int refine_edges, int device, asl_detector **out);
void asl_detector_destroy(asl_detector *det);

/* A tag family as data: the fields of upstream's apriltag_family_t that the detector reads.  Whoever has upstream's
   detector installed owns the real tables (its generated tagXXhYY.c files); this is how they are handed in.
   bit_x / bit_y follow upstream's convention: cell (0, 0) is the corner cell of the border, the border square spans
   cells 0..width_at_border-1, and a reversed-border family puts payload cells outside it (negative coordinates).
   codes[id] holds bit 0 of the family in the most significant of its nbits. */
typedef struct {
    int32_t nbits, width_at_border, total_width, reversed_border, ncodes, reserved;
    const int32_t *bit_x, *bit_y; /* nbits each */
    const uint64_t *codes;        /* ncodes */
} asl_family;

/* Whether the detector can decode `fam` exactly.  A pure host function: no GPU, no detector.  ASL_EINVAL, with
   asl_last_error() naming the field, for
     - nbits outside 1..63, or nbits % 4 not 0 or 1 (the rotation search handles nothing else);
     - width_at_border outside 2..8 (the 8 * width_at_border border samples are one per lane of a wavefront);
     - total_width above 16, below width_at_border, or total_width - width_at_border odd;
     - ncodes outside 1..65535 (the match packs the id into 16 bits);
     - a NULL array; a code with bits at or above nbits; a duplicate code;
     - a bit cell outside the total_width grid, on the border ring, on the ring of opposite colour just outside it,
       or shared by two bits;
     - a layout that does not turn with the code: bit i + nbits/4 must sit at (width_at_border - 1 - y_i, x_i), and
       with nbits % 4 == 1 the last bit at the centre cell.
   The minimum Hamming distance of the table is not checked: it is the owner's, and so is maxhamming. */
int asl_family_check(const asl_family *fam);
/* asl_detector_create for a caller's table (the other arguments as there).  The family must pass asl_family_check.
   The detector copies everything it needs: the caller's arrays may go away after the call.  The table is the caller's
   truth, so the new detector decodes all of its ids; asl_detector_set_id_limit narrows that, bounded by fam->ncodes.
   A detection carries no family field: a detector of several families (asl_detector_create_families) tells them apart
   by id ranges. */
int asl_detector_create_family(const asl_family *fam, int nthreads, int maxhamming, float decimate, float blur,
                               int refine_edges, int device, asl_detector **out);

/* Several families in one detector, decoded in one pass.  A tag with local id k of family i is reported as
   id_base[i] + k: asl_detection, asl_pose and asl_obs are what they are for one family, and the de-duplication, the
   (frame, id) order, asl_pack_observations_device, tag maps and every solver work on that global id.  Upstream's
   semantics: the quad fit's minimum tag width is the smallest of the families' max(3, width_at_border / decimate); both
   border polarities are wanted if the families' reversed_border differ; a quad is decoded against every family of its
   polarity, and every family that accepts it yields a detection of its own (two families that both accept a quad give
   two detections with different ids; there is no arbitration between families).  maxhamming is one value for all. */
#define ASL_MAX_FAMILIES 4
/* Whether asl_detector_create_families takes the set.  A pure host function, like asl_family_check.  ASL_EINVAL, with
   asl_last_error() naming the family's index and the field, for n_fams outside 1..ASL_MAX_FAMILIES, a NULL array, a
   family asl_family_check refuses, a negative id_base, two id ranges [id_base[i], id_base[i] + ncodes_i) that overlap,
   and a range that ends above 65536 (the de-duplication key holds the id in 16 bits). */
int asl_families_check(const asl_family *fams, const int32_t *id_base, int n_fams);
/* The other arguments as in asl_detector_create_family; the set must pass asl_families_check.  The detector copies what
   it needs and decodes every id of every table: asl_detector_set_id_limit on a detector of more than one family is
   ASL_EINVAL.  Everything else works as on a one-family detector (the fused PnP with its one tag_size: families printed
   at different sizes are what the per-tag sizes of a tag map are for). */
int asl_detector_create_families(const asl_family *fams, const int32_t *id_base, int n_fams, int nthreads, int maxhamming,
                                 float decimate, float blur, int refine_edges, int device, asl_detector **out);
/* Which family a reported id belongs to, and its id there.  A host function.  ASL_EINVAL for an id in no family's
   range; a one-family detector answers (0, id) for the ids of its table. */
int asl_detector_family_of(const asl_detector *det, int id, int *family_index, int *local_id);

/* Which ids the decoder may return, ASL_EINVAL beyond the detector's table.  For a detector made with
   asl_detector_create: only ids 0..4 of tagStandard41h12 are pinned by the reference (its
   assets/tags/tag{0..4}.png); upstream's 2115-entry code table is not in the reference tree, so the other
   entries of this library's built-in table are build-defined and would mislabel a physical tag with id >= 5.  Such a
   detector therefore decodes ids 0..4 only until told otherwise; to decode printed tags with id >= 5, hand upstream's
   own table to asl_detector_create_family.  n_ids <= 0 opens the whole table (synthetic scenes rendered from
   the same table), n_ids > 0 keeps ids 0..n_ids-1. */
int asl_detector_set_id_limit(asl_detector *det, int n_ids);
/* A planar tag has two poses that reproject almost equally well.  cv2.solvePnP(ITERATIVE), which the reference calls
   (tag_detector.py:41), returns the one its homography start leads to, and so does this library by default (enabled = 0).
   enabled = 1 refines the mirrored pose as well and keeps the one with the lower reprojection error (IPPE's
   two-solution test): better orientation for small, near-frontal tags, but no longer what the reference computes. */
int asl_detector_set_pnp_both_minima(asl_detector *det, int enabled);
/* Upstream's quad_sigma (the `blur` keyword of its Python wrapper): > 0 blurs the decimated image with a Gaussian of that
   sigma before the threshold, < 0 sharpens it (2 * image - blurred, clipped); 0 = off, the default.  The threshold,
   the segmentation and the quad fit then read the filtered image; edge refinement and decoding keep sampling the
   original frame, as upstream.  The kernel has ksz = int(4 * |quad_sigma|) taps, made odd; a sigma whose ksz is 1 is
   accepted and is off.  ASL_EINVAL for a non-finite value, for |quad_sigma| >= 4 (ksz <= 15) and while a batch is pending
   (between submit and collect).  Takes effect from the next batch, on every detect entry point. */
int asl_detector_set_quad_sigma(asl_detector *det, float quad_sigma);
/* The taps asl_detector_set_quad_sigma(quad_sigma) filters with: uint8 = floor(255 * normalised Gaussian), *ksz of them
   (0 = off) into taps[max_taps].  A pure host function: no GPU, no detector.  ASL_EINVAL, nothing written, for a
   quad_sigma the setter refuses or max_taps < *ksz. */
int asl_blur_taps(float quad_sigma, uint8_t *taps, int max_taps, int *ksz);
const char *asl_last_error(void);
/* "aprilslam <version> gfx950 ..." */
const char *asl_version(void);

/* Replaces detector.detect(gray) (reference tag_detector.py:26).  Host image in, detections
   (sorted by id) out.  *n_out = number found; at most max_out are written. */
int asl_detect_gray_u8(asl_detector *det, const uint8_t *gray, int w, int h, int stride,
                       asl_detection *out, int max_out, int *n_out);
/* Replaces cv2.cvtColor(BGR2GRAY) + detector.detect (reference tag_detector.py:25-27): the
   gray conversion is fused into the first kernel. */
int asl_detect_bgr_u8(asl_detector *det, const uint8_t *bgr, int w, int h, int stride,
                      asl_detection *out, int max_out, int *n_out);

/* Batched form of the two calls above: n_frames host images of identical geometry.
   channels = 1 (gray) or 3 (BGR).  out holds up to max_out detections in total, ordered by
   (frame, id); n_per_frame[n_frames] receives the count for each frame. */
int asl_detect_batch_u8(asl_detector *det, const uint8_t *const *frames, int n_frames, int channels,
                        int w, int h, int stride, asl_detection *out, int max_out, int *n_per_frame,
                        int *n_out);

/* asl_detect_batch_u8 with the per-tag PnP (asl_solve_pnp_batch) fused into the same submission: what the reference
   does per frame with detector.detect + one cv2.solvePnP per tag (tag_detector.py:26,41) in a single call.
   poses[i] belongs to out[i]; K is 9 doubles row-major; dist holds n_dist = 0, 4 or 5 coefficients. */
int asl_detect_batch_pose_u8(asl_detector *det, const uint8_t *const *frames, int n_frames, int channels,
                             int w, int h, int stride, const double *K, const double *dist, int n_dist,
                             double tag_size, asl_detection *out, asl_pose *poses, int max_out,
                             int *n_per_frame, int *n_out);

/* Same, frames already resident in HBM: frame i starts at d_frames + i*frame_pitch.
   If K is non-NULL the per-tag PnP (asl_solve_pnp_batch) runs on the device in the same
   submission and poses[i] belongs to out[i].  Results are written to HOST memory; the call
   returns after the stream has drained. */
int asl_detect_batch_device(asl_detector *det, const void *d_frames, int n_frames, int channels,
                            int w, int h, int stride, size_t frame_pitch, void *stream,
                            const double *K /*9, row-major, or NULL*/, const double *dist, int n_dist,
                            double tag_size, asl_detection *out, asl_pose *poses, int max_out,
                            int *n_per_frame, int *n_out);

/* The same call split in two so that batches can be pipelined: submit enqueues the whole batch (kernels and
   the asynchronous read-back) on `stream` and returns immediately; collect waits for it, de-duplicates and
   writes the results.  One batch may be in flight per detector; use two detectors (two workspaces) and
   alternate them to keep the GPU busy while the host post-processes the previous batch. */
int asl_submit_batch_device(asl_detector *det, const void *d_frames, int n_frames, int channels, int w, int h,
                            int stride, size_t frame_pitch, void *stream, const double *K, const double *dist,
                            int n_dist, double tag_size);
int asl_collect_batch(asl_detector *det, asl_detection *out, asl_pose *poses, int max_out, int *n_per_frame,
                      int *n_out);
/* The same without the last copy: *out / *poses / *n_per_frame point into the detector's own page-locked result buffers
   (*n_out detections in (frame, id) order, *poses = NULL for a batch submitted without a camera); they stay valid until
   the next submit on this detector. */
int asl_collect_batch_view(asl_detector *det, const asl_detection **out, const asl_pose **poses, const uint32_t **n_per_frame,
                           int *n_out);

/* Replaces cv2.solvePnP(ITERATIVE) + cv2.Rodrigues for N tags at once (reference
   tag_detector.py:30-52).  corners: N x 4 x 2 float32 (lb,rb,rt,lt), K row-major 3x3,
   dist: n_dist in {0,4,5} coefficients (k1,k2,p1,p2[,k3]).  All pointers are host memory.
   A tag without a pose (degenerate or non-finite corners) has ok = 0 and zeros in all of its rvec, tvec and T, whatever
   it shares a wavefront with; an asl_pose with ok = 0 from the detect calls with a camera holds the same zeros. */
int asl_solve_pnp_batch(asl_detector *det, const float *corners, const double *K, const double *dist,
                        int n_dist, double tag_size, double *rvec /*N x 3*/, double *tvec /*N x 3*/,
                        double *T /*N x 16*/, uint8_t *ok /*N*/, int N);

/* Pose-graph Gauss-Newton back-end (NOT in the reference: slam_graph.py:72-76 is a stub).
   Unknowns: n_cams camera poses and n_tags tag poses (world<-x 4x4, row-major, updated in
   place); tag `fixed_tag` is held at its input value and defines the world frame.
   Observation k: camera obs_cam[k] saw tag obs_tag[k] with pixel corners obs_corners[k] (4x2).
   Residual: the 8 pixel reprojection errors of the tag's 4 corners.  Runs `iters`
   Levenberg-Marquardt steps on the device; stats[0] = initial cost, stats[1] = final cost,
   stats[2] = iterations accepted. */
int asl_gn_solve(asl_detector *det, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam,
                 const int32_t *obs_tag, const double *obs_corners, const double *K, double tag_size,
                 int fixed_tag, double *cam_T /*n_cams x 16*/, double *tag_T /*n_tags x 16*/, int iters,
                 double *stats /*3*/);

/* ---- after the detector: what the multi-GPU path exchanges and how the graph update consumes it.
   One observation = one detected tag of one frame: what SLAM.get_pose hands to SLAMGraph.add_or_update_node
   (reference slam.py:27-32) plus the corners a later bundle adjustment needs. */
typedef struct {
    int32_t id;       /* -1 = empty slot */
    int32_t flags;    /* bit 0: slot used; bit 1: solvePnP succeeded (the reference updates the graph only then) */
    float corners[8]; /* lb, rb, rt, lt in pixels, float32 as the reference passes them to solvePnP */
    double T[12];     /* rows 0..2 of the camera<-tag 4x4 (row 3 is 0 0 0 1) */
} asl_obs;            /* 136 bytes */

/* Packs the de-duplicated results of the batch last submitted on `det` into d_obs (device memory,
   n_frames x max_tags records, slots ordered by id, empty slots id = -1) on `stream` -- no host round trip, so the
   block can go straight into an all-gather.  Call between asl_submit_batch_device and the next submit. */
int asl_pack_observations_device(asl_detector *det, void *d_obs, int max_tags, void *stream);

/* The data-parallel part of the graph update over gathered records d_obs[world][n_frames][max_tags]:
   d_pose[world*n_frames][16] = SLAM.my_pose() of every frame that (a) sees the world tag `coordinate_id` as its lowest id
   and (b) has no failed PnP -- such a frame's update depends on nothing but the frame (branches A / C1 of
   slam_graph.py:33-49); d_status = 0 for those, 1 for frames that need the sequential update, 2 for frames without
   detections; d_last[id] (caller zeroes it) = 1 + ((frame*world + stream)*max_tags + slot) of the last status-0 frame,
   in (frame, stream) order, that saw tag `id`; d_picks (optional, 2*n_ids asl_obs) receives for every such tag its
   record in that frame and the frame's world-tag record -- all the host needs to finish the update without touching
   the block again. */
int asl_graph_frames_device(asl_detector *det, const void *d_obs, int world, int n_frames, int max_tags, int coordinate_id,
                            double *d_pose, uint8_t *d_status, uint32_t *d_last, int n_ids, void *d_picks, void *stream);

/* Last sightings and picks as above, restricted to the status-0 frames whose position frame*world + stream lies in
   [order_lo, order_hi) (d_status from asl_graph_frames_device; d_last is zeroed here).  The host applies the
   self-contained stretches of a block between two frames that need the sequential update with it
   (aprilslam_amd/dist.py: apply_block). */
int asl_graph_picks_device(asl_detector *det, const void *d_obs, int world, int n_frames, int max_tags, const uint8_t *d_status,
                           unsigned int order_lo, unsigned int order_hi, uint32_t *d_last, int n_ids, void *d_picks, void *stream);

/* ---- after the detector: the camera pose of every frame from all its tags against a known map of tag poses (a "tag bundle").
   The map may come from the pose-graph back-end, from a survey or from a synthetic scene. */
typedef struct {
    double T[12];    /* world<-tag, rows 0..2 of the 4x4 (the tag frame of asl_pose: corners (+-h, +-h, 0), lb rb rt lt) */
    int32_t valid;   /* 0: no pose for this id */
    float size;      /* the side of this tag, in the units and with the meaning of tag_size (between the corner points the
                        detector reports).  0: the call's tag_size (every map asl_map_* writes).  > 0 and finite: this tag's
                        own side; its corners are (+-h_id, +-h_id, 0) with h_id = size * 0.5f.  Negative or not finite: the
                        entry counts as valid = 0 */
} asl_map_tag;       /* indexed by tag id; 104 bytes */

/* Every entry point below that takes d_map / map honours the entries' sizes: localisation, the rig forms, their covariances,
   calibration and the sequence solves.  Their tag_size is the size of the entries whose size is 0.  The per-tag PnP poses in
   the records (asl_obs.T) are taken as solved at tag_size: the seed of a sized tag uses that pose with its translation
   times size / tag_size (object and translation scaled together leave every ray where it is, under any lens). */

typedef struct {
    double T[16];        /* world<-camera, row-major (the convention of asl_gn_solve's cam_T) */
    double rms_px;       /* final reprojection RMS (pixels per corner) over the slots used */
    double rms_seed_px;  /* the same of the winning candidate before refinement, over every slot that took part */
    int32_t n_tags;      /* slots used in the final solve */
    int32_t n_rejected;  /* slots dropped by the gate */
    int32_t status;      /* 0 ok, 1 no mapped tag in view, 2 no slot with a successful PnP */
    int32_t seed_slot;   /* slot of the winning candidate; +256 if it was the mirrored one; -1 if none */
} asl_cam_pose;          /* 160 bytes */

/* One camera pose per frame of d_obs (n_frames x max_tags records as asl_pack_observations_device writes them), device
   pointers, asynchronous on `stream`.  A slot takes part if flags & 1 and its id has a valid map entry (id < n_ids); its
   4 corners are residuals against the map tag's corners (tag_size is the size of the entries whose size is 0).  The seed is the best, over all taking-part corners, of the
   poses that the PnP of the <= 8 largest slots with flags & 2 imply through the map, each also in its mirrored planar
   minimum; Levenberg-Marquardt on the 6 pose parameters refines it (K 9 doubles row-major, dist n_dist = 0, 4 or 5
   coefficients, as asl_solve_pnp_batch).  max_tag_rms_px > 0 is an outlier gate: while the slot of largest own corner RMS
   exceeds it, that slot is dropped and the solve runs again (one slot at a time, at most 8, never the last); 0 turns it off.  max_tags in [1, 256]; deterministic: the same input gives the same bytes. */
int asl_localize_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                               const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                               void *d_out, void *stream);
/* The same computation on host records, synchronous (the detector keeps the device copies and grows them on demand). */
int asl_localize_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                       const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                       asl_cam_pose *out);

/* ---- how good a pose is: its first-order (Gauss-Newton) covariance C = sigma^2 (J^T J)^-1 at the solution the solver
   returned, J the Jacobian of the pixel residuals that solver minimised.
   Convention: for a pose T = [R | p] the error is (r, d) with R_true = Rod(r) R and p_true = p + d.  So the lower 3x3
   block is the covariance of the translation column itself (the camera position in world axes for world<-camera, tvec
   for camera<-tag) and the upper block that of the rotation error about the axes of the pose's target frame (world /
   camera).  This is not the (omega, v) of a left update T_true = [Rod(omega) | v] T that d_tag_std reports: there
   p_true = Rod(omega) p + v, so the v of a pose far from the origin carries the lever arm omega x p.  To first order
   r = omega, d = v - [p]x omega, i.e. (r, d) = A (omega, v) with A = [I 0; -[p]x I] and C_(r,d) = A C_(omega,v) A^T.
   (The solvers update camera<-X by (w, v) on the left; camera<-tag is that pose itself, A as above with p = tvec;
   world<-camera is its inverse, r = -R_cx^T w, d = -R_cx^T v.)  tests/pose_cov_ref.py states the computation.
   sigma_px > 0: the corner noise (pixels, per coordinate) the caller assumes.  sigma_px == 0: estimated from the solve,
   sigma^2 = cost / dof with dof = 8 n_tags - 6.  For one tag that is 2 degrees of freedom: the estimate is then itself
   uncertain by a factor of about two either way, and a given sigma_px is the better choice.  A covariance is as good as
   the model: independent Gaussian corner noise, a linearisation that holds over the error, and (localisation) a map taken
   as exact -- asl_localize_cov_* and asl_localize_rig_cov_* do not propagate the uncertainty of the map tags, which for a
   map built by asl_map_* is most of the pose's error; asl_localize_mapcov_* below do, from the map's joint covariance. */
typedef struct {
    double cov[36];     /* row-major 6x6, symmetric to the bit, order (rx ry rz | px py pz) */
    double sigma_px;    /* the pixel sigma that scaled it (given, or estimated) */
    int32_t dof;        /* residuals - 6 of the solve it belongs to (0 with status 1) */
    int32_t status;     /* 0 ok; 1 the pose has none (its own status != 0 / PnP not ok); 2 J^T J not positive definite;
                           3 (asl_localize_mapcov_* only) a d_cov_slot entry of a slot in the solve outside [-1, ld / 6), or a
                           block of d_map_cov that is not finite */
} asl_pose_cov;         /* 304 bytes; status != 0: cov all zero */

/* asl_localize_frames_device with the covariance of every frame's world<-camera pose: d_out receives exactly what
   asl_localize_frames_device writes, byte for byte; d_cov one asl_pose_cov per frame, over the slots in the final solve
   (after the gate), computed in the same kernel from the corners still on chip.  sigma_px < 0 or non-finite is
   ASL_EINVAL.  Deterministic: the same input gives the same bytes. */
int asl_localize_cov_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                   const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                   double sigma_px, void *d_out, void *d_cov, void *stream);
/* The same computation on host records, synchronous. */
int asl_localize_cov_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                           const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                           double sigma_px, asl_cam_pose *out, asl_pose_cov *cov);

/* asl_localize_cov_frames_device with the uncertainty of the map carried into the pose covariance.  d_map_cov (doubles,
   row-major, leading dimension ld, a positive multiple of 6) and d_cov_slot (n_ids int32: the block of every id, -1 for an
   id without one, which is then exact) are what asl_mapcov_frames_device writes, and may be handed over on the same stream
   without a host copy.  d_out is byte for byte what the plain call writes.  Over the slots s in the final solve (after the
   gate), tag j(s), at the returned pose (R, t) = camera<-world: J_s (8 x 6) the rows the solver forms,
   Jp [-[p_c]x | I]; M_s (8 x 6) the rows of the same residuals over the tag's (omega, v), Jp R [-[X]x | I], X the world
   corner; A = sum J_s^T J_s, N_s = J_s^T M_s, Q = sum over s, s' with a block of N_s Sigma[j(s), j(s')] N_s'^T, and
   C = sigma^2 A^-1 + A^-1 Q A^-1, mapped to the world<-camera (r, d) convention above like the plain covariance; sigma and
   dof as there.  With every slot -1 the record is byte for byte asl_localize_cov_frames_device's.  status 3 (zeros; the
   pose is untouched): see asl_pose_cov.  The pair sum runs in a fixed order: the same input gives the same bytes;
   max_tags = 256 with every slot in the solve is 65,536 pairs a frame.  ASL_EINVAL, nothing written: whatever
   asl_localize_cov_frames_device refuses; d_map_cov or d_cov_slot NULL; ld < 6 or not a multiple of 6.  Mountings,
   intrinsics and tag sizes stay exact.  tests/localize_mapcov_ref.py states the computation. */
int asl_localize_mapcov_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                      const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                                      double sigma_px, void *d_out, void *d_cov, const void *d_map_cov, int ld,
                                      const void *d_cov_slot, void *stream);
/* The same computation on host records, synchronous.  The host form also refuses (ASL_EINVAL, nothing written) what the
   device form can only report as status 3: a cov_slot entry outside [-1, ld / 6), or an entry of the blocks the slots
   refer to that is not finite. */
int asl_localize_mapcov_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                              const double *K, const double *dist, int n_dist, double tag_size, double max_tag_rms_px,
                              double sigma_px, asl_cam_pose *out, asl_pose_cov *cov, const double *map_cov, int ld,
                              const int32_t *cov_slot);

/* ---- several cameras on one rigid body (a "rig") localised together: one pose rig<-world per frame, every camera's
   corners in one solve.  Camera c has its own model (K, dist: as asl_solve_pnp_batch) and a fixed mounting
   E = camera_c<-rig; a world corner X seen by camera c contributes project_c(E_c (rig<-world) X) - pixel.  The rig frame
   is whatever frame the mountings are given in (Rig.from_camera_poses: camera 0). */
typedef struct {
    double K[9];      /* row-major */
    double dist[5];   /* k1 k2 p1 p2 k3; unused = 0 (entries past n_dist are not read) */
    double E[12];     /* camera<-rig, rows 0..2 of the 4x4 */
    int32_t n_dist;   /* 0, 4 or 5 */
    int32_t reserved;
} asl_rig_camera;     /* 216 bytes */

/* asl_localize_frames_device for a rig.  d_obs: n_cams x n_frames x max_tags records, camera-major (what
   all_gather_into_tensor makes of the ranks' packed blocks, or asl_pack_observations_device called once per camera at
   d_obs + c * n_frames * max_tags records); frame f of every camera is one instant.  The frame's records are its global
   slots g = c * max_tags + s, and gather, seed, refinement and gate are those of asl_localize_frames_device over global
   slots: the seeds are the <= 8 global slots with flags & 2 of largest corner area -- in pixels squared as they are, so
   cameras of different focal length are not put on one scale -- and a seed of camera c implies the rig pose
   inv(E_c) T_obs inv(map[id]), scored over the taking-part corners of all cameras.  tag_size is one value for the rig
   (the size of the map entries whose size is 0).
   d_out: one asl_cam_pose per frame with T = world<-rig; n_tags / n_rejected count global slots, status 1: no mapped tag
   in any camera, 2: no slot with a successful PnP, seed_slot the global slot of the winner (+256 if mirrored).  A rig of
   one camera with E = identity is asl_localize_frames_device.
   d_rig: n_cams asl_rig_camera in device memory; it is read back and checked before the launch (the one synchronous
   step), so it must be complete when the call is made.  n_cams in [1, 16], max_tags in [1, 256],
   n_cams * max_tags <= 256; a camera with n_dist not 0 / 4 / 5, a non-finite K or E or an E whose rotation part is not
   orthonormal to 1e-6 is ASL_EINVAL.  Deterministic: the same input gives the same bytes. */
int asl_localize_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                   int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px, void *d_out, void *stream);
/* With the covariance of every frame's world<-rig pose (asl_pose_cov, dof = 8 n_tags - 6), as
   asl_localize_cov_frames_device: d_out byte for byte what the plain call writes.  The mountings and the map are taken as
   exact: their uncertainty is not propagated (the map's: asl_localize_rig_mapcov_frames_device below). */
int asl_localize_rig_cov_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                       int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                       void *d_out, void *d_cov, void *stream);
/* The same computations on host records, synchronous (the detector keeps the device copies and grows them on demand). */
int asl_localize_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                           int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, asl_cam_pose *out);
int asl_localize_rig_cov_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                               int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, double sigma_px,
                               asl_cam_pose *out, asl_pose_cov *cov);

/* asl_localize_rig_cov_frames_device with the map's joint covariance carried into the covariance of the world<-rig pose,
   as asl_localize_mapcov_frames_device: R is the rotation of E_c (rig<-world) for the view's camera, J_s the rows over the
   rig pose as the solver forms them.  The mountings stay exact. */
int asl_localize_rig_mapcov_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags,
                                          const void *d_map, int n_ids, const void *d_rig, double tag_size, double max_tag_rms_px,
                                          double sigma_px, void *d_out, void *d_cov, const void *d_map_cov, int ld,
                                          const void *d_cov_slot, void *stream);
int asl_localize_rig_mapcov_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                                  int n_ids, const asl_rig_camera *rig, double tag_size, double max_tag_rms_px, double sigma_px,
                                  asl_cam_pose *out, asl_pose_cov *cov, const double *map_cov, int ld, const int32_t *cov_slot);

/* ---- tag bundles: several rigid objects that each carry a few tags (a tool, a pallet, a landing pad, other robots), every
   one posed in every frame by one launch.  Bundle b is a table of n_ids asl_map_tag with T = bundle_b<-tag, the object's
   tag layout in its own frame (valid = 0 for the ids it does not carry; sizes honoured as everywhere); d_maps holds the
   n_bundles tables one after another, table b at d_maps + b * n_ids records.  The grid is (frame, bundle): one wavefront
   solves frame f against table b exactly as asl_localize_frames_device does with that table as its map -- "world<-camera"
   with the bundle as the world -- and writes record f * n_bundles + b.
   Contract: record (f, b) of d_out, and of d_cov where given, is byte for byte what asl_localize_frames_device /
   asl_localize_cov_frames_device writes for frame f when called with table b alone: T = bundle_b<-camera, gate, statuses
   and seed_slot included.  A frame that sees no tag of bundle b gets status 1 (the common case, and the solve's first
   exit).  d_cov NULL: the plain solve (sigma_px is checked and not used); else n_frames x n_bundles asl_pose_cov, sigma_px
   as in asl_localize_cov_frames_device.  The covariances take the layouts as exact: a bundle's own uncertainty (a table
   cut from a map asl_map_* built) is not propagated, and there are no mapcov forms for bundles.
   ASL_EINVAL, nothing written: whatever the one-map calls refuse; n_bundles outside [1, 1024]; n_frames * n_bundles past
   2^31 - 1.  Nothing waits that the one-map forms do not wait for.  Deterministic: the same input gives the same bytes.
   The library does not look for an id that is valid in two tables (see asl_bundle_relative_device); bundles.BundleSet of
   the Python layer refuses one. */
int asl_localize_bundles_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_maps,
                                       int n_bundles, int n_ids, const double *K, const double *dist, int n_dist, double tag_size,
                                       double max_tag_rms_px, double sigma_px, void *d_out, void *d_cov, void *stream);
/* The same computation on host records, synchronous: maps is n_bundles x n_ids records, out and cov (NULL: plain)
   n_frames x n_bundles. */
int asl_localize_bundles_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *maps,
                               int n_bundles, int n_ids, const double *K, const double *dist, int n_dist, double tag_size,
                               double max_tag_rms_px, double sigma_px, asl_cam_pose *out, asl_pose_cov *cov);
/* For a rig: asl_localize_rig_frames_device / asl_localize_rig_cov_frames_device per (frame, bundle) under the same contract,
   T = bundle_b<-rig.  The table d_rig is read back and checked before the launch, the one synchronous step, as there. */
int asl_localize_bundles_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags,
                                           const void *d_maps, int n_bundles, int n_ids, const void *d_rig, double tag_size,
                                           double max_tag_rms_px, double sigma_px, void *d_out, void *d_cov, void *stream);
int asl_localize_bundles_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags,
                                   const asl_map_tag *maps, int n_bundles, int n_ids, const asl_rig_camera *rig, double tag_size,
                                   double max_tag_rms_px, double sigma_px, asl_cam_pose *out, asl_pose_cov *cov);

/* The pose of bundle b in the frame of a reference bundle, per frame, from what the calls above wrote. */
typedef struct {
    double T[16];      /* ref<-bundle_b, row-major 4x4 */
    double cov[36];    /* its covariance in the (r, d) convention of asl_pose_cov, row-major 6x6, symmetric to the bit */
    int32_t status;    /* 0 ok; 1 bundle b or the reference has no pose in this frame (its asl_cam_pose.status != 0): T identity,
                          cov zeros; 2 both poses ok, but d_cov is NULL or one of the two asl_pose_cov.status != 0: T valid, cov
                          zeros */
    int32_t reserved;  /* written 0 */
} asl_bundle_rel;      /* 424 bytes */

/* d_poses: n_frames x n_bundles asl_cam_pose (record f * n_bundles + b: T_b = bundle_b<-camera, or bundle_b<-rig); d_cov:
   as many asl_pose_cov, or NULL; ref in [0, n_bundles).  d_rel: one asl_bundle_rel per (frame, bundle).  Device pointers,
   asynchronous on `stream`; one lane per record, float64, no atomics, a fixed order of operations: the same input gives
   the same bytes.  With a = ref, T_a = [R_a | p_a] and T_b = [R_b | p_b]:
       R_ab = R_a R_b^T,  q = R_ab p_b,  p_ab = p_a - q                               (T_ab = T_a inv(T_b))
       r_ab = r_a - R_ab r_b,  d_ab = d_a + [q]x r_ab - R_ab d_b                      (to first order)
       J_a = [I 0; [q]x I],  J_b = [-R_ab 0; -[q]x R_ab  -R_ab],  C_ab = J_a C_a J_a^T + J_b C_b J_b^T
   (built as J_a (C_a + D C_b D^T) J_a^T with D = diag(R_ab, R_ab), which is the same matrix; the Jacobians agree with
   central differences of the exact composition, tests/test_bundle_ref.py).  b == ref: the identity, zero covariance,
   status 0 or 1 by the reference's pose.
   The sum takes the two poses as independent, which they are when their solves share no corner: an id that is valid in
   two tables breaks that, and the covariance is then too small or too large by the shared part.  As in the solves, the
   layouts are exact: the uncertainty of the bundles' own tables is not propagated.
   ASL_EINVAL, nothing written: NULL det, d_poses or d_rel; n_frames < 0; n_bundles outside [1, 1024]; n_frames * n_bundles
   past 2^31 - 1; ref outside [0, n_bundles).  tests/bundle_ref.py states the computation. */
int asl_bundle_relative_device(asl_detector *det, const void *d_poses, const void *d_cov, int n_frames, int n_bundles, int ref,
                               void *d_rel, void *stream);
/* The same computation on host records, synchronous. */
int asl_bundle_relative_batch(asl_detector *det, const asl_cam_pose *poses, const asl_pose_cov *cov, int n_frames, int n_bundles,
                              int ref, asl_bundle_rel *rel);

/* One asl_pose_cov per asl_obs record (n_records of them, as asl_pack_observations_device writes them; device pointers,
   asynchronous on `stream`): the covariance of the camera<-tag pose in the record from its 4 corners (8 residuals, dof 2),
   re-linearised at that pose with the camera model of asl_solve_pnp_batch.  Records without flags & 2 get status 1.
   The fused detect + PnP has no covariance output: the device path is submit -> pack -> this call. */
int asl_pose_cov_device(asl_detector *det, const void *d_obs, int n_records, const double *K, const double *dist, int n_dist,
                        double tag_size, double sigma_px, void *d_cov, void *stream);
/* The same on what asl_solve_pnp_batch took and returned (host pointers, synchronous): corners N x 4 x 2 float32,
   T N x 16.  A T with a non-finite entry in its first three rows (a failed PnP) gets status 1. */
int asl_solve_pnp_cov_batch(asl_detector *det, const float *corners, const double *T, const double *K, const double *dist,
                            int n_dist, double tag_size, double sigma_px, asl_pose_cov *cov, int N);

/* ---- camera calibration from tag observations: intrinsics and lens distortion of the camera model above (fx fy cx cy,
   k1 k2 p1 p2 [k3]) from frames that see a rigid target of known tag poses (a planar board or any surveyed arrangement). */
#define ASL_CALIB_FIX_PRINCIPAL_POINT 1  /* cx, cy stay at K_init's (or the image centre) */
#define ASL_CALIB_FIX_ASPECT_RATIO    2  /* fx = r fy, r = fx / fy of K_init (1 without) */
#define ASL_CALIB_ZERO_TANGENT_DIST   4  /* p1 = p2 = 0 */
typedef struct {
    double K[9];          /* row-major */
    double dist[5];       /* k1 k2 p1 p2 k3; unused = 0 */
    double std[9];        /* fx fy cx cy k1 k2 p1 p2 k3; fixed / unused = 0 */
    double rms_px;        /* final, per corner, over the frames used */
    double rms_init_px;   /* after the seed, with K0 and no distortion */
    int32_t n_frames_used, n_corners, iterations;
    int32_t status;       /* 0 ok, 1 too few frames/corners, 2 no closed-form focal length, 3 solve failed (non-finite) */
} asl_calib_result;       /* 216 bytes */

/* Calibrate from d_obs (n_frames x max_tags records as asl_pack_observations_device writes them; only flags & 1, id and
   corners are read -- the PnP pose in the record was computed with some other K) against d_map (n_ids asl_map_tag;
   tag_size is the size of the entries whose size is 0, and a sized tag's planar pose is formed at its own half).
   A frame takes part with >= 2 mapped slots.  Without K_init the principal point starts at (width / 2, height / 2) and
   the focal lengths come in closed form from every tag's homography (Zhang's constraints, least squares); each frame is
   seeded with that K0 and no distortion (planar pose of its <= 8 largest tags and their mirrored minima, scored over all
   its corners, then pose-only LM), then Levenberg-Marquardt refines the n_dist = 0, 4 or 5 coefficients, the free
   intrinsics and every frame's pose together, each frame eliminating its pose block (Schur complement).  std is
   sqrt(sigma^2 diag(S^-1)) at the solution.  d_result: one asl_calib_result; d_poses: n_frames asl_cam_pose, world<-camera,
   rms_px final, rms_seed_px after the seed, n_tags, status 0 used, 1 fewer than 2 mapped slots, 3 dropped (every seed
   candidate had a corner behind the camera), 4 taking part in a calibration that failed.  The whole solve (max_iters >= 1
   trials) is enqueued on `stream` without a wait; max_tags in [1, 256]; deterministic: the same input gives the same
   bytes.  tests/calib_ref.py states the algorithm. */
int asl_calibrate_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                double tag_size, int width, int height, const double *K_init /* 9 or NULL */, int n_dist,
                                int flags, int max_iters, void *d_result, void *d_poses, void *stream);
/* The same computation on host records, synchronous (the detector keeps the device copies and grows them on demand). */
int asl_calibrate_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                        double tag_size, int width, int height, const double *K_init, int n_dist, int flags, int max_iters,
                        asl_calib_result *result, asl_cam_pose *poses);

/* ---- rig mounting calibration: the mountings E_c = camera_c<-rig of a rig's cameras, refined jointly with one rig pose
   per frame from the frames of a known tag map that two or more cameras see.  Every rig solver takes the mountings as
   exact; this is the call that produces them (Rig.from_camera_poses averages single-camera poses and refines nothing). */
typedef struct {
    double rms_px;          /* final, per corner, over the frames used */
    double rms_init_px;     /* the same frames at their seed poses under the mountings as given */
    double sigma_px;        /* the pixel sigma that scaled the covariances (given, or estimated) */
    int32_t n_frames_used, n_corners, iterations;
    int32_t status;         /* 0 ok, 1 nothing to solve (no solved camera, or too few corners), 3 solve failed */
    int32_t n_solved, reserved;
    int32_t cam_status[16]; /* 0 solved, 1 the reference camera, 2 held (not connected to it); 0 past n_cams */
    int32_t cam_frames[16]; /* the used frames in which the camera has a taking-part slot */
} asl_rig_calib_result;     /* 176 bytes */

/* d_obs, d_map, tag_size as for asl_localize_rig_frames_device; d_rig: n_cams asl_rig_camera whose E are the INITIAL
   mountings (read back and checked before anything is enqueued, the one synchronous step).  Every frame is first
   localised under those mountings with the gate off (exactly what asl_localize_rig_frames_device writes).  mask(f) is the
   set of cameras with a taking-part slot (flags & 1, a valid map entry) in a frame whose seed has status 0.  Starting from
   {camera 0}, a frame with two or more cameras in its mask, one of them reached, reaches them all (n_cams - 1 sweeps).
   Used frames: two or more cameras, all reached.  Solved cameras: the reached ones but camera 0, whose E is the gauge and
   stays as given (it need not be the identity).  A camera that is not reached is held: its mounting cannot be observed,
   and its E comes back byte for byte.
   Levenberg-Marquardt then refines the solved mountings (left update E <- [Rod(w) | v] E) and every used frame's pose
   together, each frame eliminating its pose block (Schur complement), the reduced system (<= 42 x 42) solved by Cholesky;
   the schedule is asl_calibrate_frames_device's (lambda0 1e-3, x0.1 / x10, at most max_iters >= 1 trials, stop at a
   relative decrease below 1e-12).  There is no outlier gate: pass clean observations.
   d_rig_out: n_cams asl_rig_camera, K / dist / n_dist copied, E refined for the solved cameras; it may be d_rig.
   d_result: one asl_rig_calib_result; with status 1 or 3 d_rig_out equals d_rig.
   d_cov: n_cams asl_pose_cov of the pose E_c in the (r, d) convention above, from sigma^2 S^-1 of the undamped reduced
   system at the solution (sigma_px == 0: sigma^2 = cost / dof, dof = 2 n_corners - 6 n_frames_used - 6 n_solved, which is
   the dof written); status 1 (zeros, dof 0) for camera 0, for held cameras and whenever the result status is not 0.
   Covariances between cameras are not reported.
   d_poses: n_frames asl_cam_pose, world<-rig.  Used frames: the refined pose, status 0, rms_px final, rms_seed_px and
   seed_slot of the seed, n_tags the taking-part slots.  Other frames: the seed's record, status 5 where the seed's was 0
   (localised under the initial mountings, outside the joint solve: asl_localize_rig_* with d_rig_out re-localises them),
   else its 1 or 2.  Result status 1: every frame is such a frame; 3: the used frames keep the seed's record, status 4.
   n_cams in [2, 8], max_tags in [1, 256], n_cams * max_tags <= 256, n_frames >= 1; sigma_px < 0 or non-finite, a bad
   table or a NULL pointer is ASL_EINVAL, and nothing is written or enqueued.  The whole solve is enqueued on `stream`
   without a wait; deterministic: the same input gives the same bytes.  tests/rig_calib_ref.py states the algorithm. */
int asl_calibrate_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                    int n_ids, const void *d_rig, double tag_size, int max_iters, double sigma_px, void *d_rig_out,
                                    void *d_result, void *d_cov, void *d_poses, void *stream);
/* The same computation on host records, synchronous (the detector keeps the device copies and grows them on demand). */
int asl_calibrate_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                            int n_ids, const asl_rig_camera *rig, double tag_size, int max_iters, double sigma_px,
                            asl_rig_camera *rig_out, asl_rig_calib_result *result, asl_pose_cov *cov, asl_cam_pose *poses);

/* ---- tag-map reconstruction: the world<-tag pose of every tag a batch of frames sees, every frame's camera pose and a
   per-tag std, from the asl_obs block alone (no map given).  The output is the asl_map_tag block
   asl_localize_frames_device reads. */
typedef struct {
    double cost_seed, cost;        /* sum of squared pixel residuals after the seed / at the end */
    double rms_px, rms_seed_px;    /* per corner, over the observations in the solve */
    int32_t n_frames_used, n_tags, n_obs, n_obs_dropped;  /* n_tags counts the world tag; n_obs_dropped: taking-part slots
                                                             of frames with >= 2 of them that are not in the solve */
    int32_t iterations;            /* LM trials run */
    int32_t world_id;
    int32_t status;                /* 0 ok, 1 nothing to solve (no world tag in a used frame, or no observation left),
                                      2 reduced system not positive definite, 3 non-finite */
    int32_t n_soft;                /* asl_map_robust_*: observations in the solve with a corner over the Huber threshold at the
                                      returned poses; 0 from the plain calls */
} asl_map_result;                  /* 64 bytes */

/* Map from d_obs (n_frames x max_tags records as asl_pack_observations_device writes them), device pointers.  A slot takes
   part if flags & 1 and 0 <= id < n_ids (a repeated id only in its first slot); a frame is used with >= 2 such slots.  The
   tags are the ids seen in used frames; world_id (-1: the lowest of them) is the identity of the map.  Seed: breadth-first
   rounds from the world tag through the largest flags & 2 observation (ties: lower tag id / lower frame), two reseed sweeps
   (cameras, then tags: the current pose, or the pose the PnP of one of the <= 8 largest flags & 2 observations implies, or
   its mirrored planar minimum, whichever has the least total reprojection error), the world tag back at the identity, a
   flip test per tag (its pose against its mirror, each polished by pose-only LM).  An observation with a corner at
   z <= 1e-6 in its camera then leaves; a frame with fewer than 2 left is dropped.  Joint Levenberg-Marquardt over 6
   parameters per frame and per tag but the world tag, the camera model of asl_solve_pnp_batch (K, n_dist = 0, 4 or 5
   coefficients, corners (+-h, +-h, 0), h = float32(tag_size / 2)), at most max_iters trials (in [1, 1000]; all of them are
   enqueued, and after the stop each remaining one still factors an identity system of the reduced size), stopping on an
   accepted trial of relative decrease below 1e-12.  d_map: n_ids asl_map_tag, world<-tag, valid for the mapped tags; d_tag_std (NULL:
   skipped): n_ids x 6 doubles, sqrt(sigma^2 diag) of the tag's block of the inverse undamped normal matrix, (omega, v) of a
   left update in the world frame, sigma^2 = cost / (8 n_obs - 6 frames - 6 (tags - 1)), 0 for the world tag and unmapped
   ids, and 0 for every tag if the undamped reduced system at the solution is not positive definite; d_poses: n_frames asl_cam_pose, world<-camera, rms_px final and rms_seed_px after the seed over the frame's
   observations in the solve, n_tags those, n_rejected the rest of its taking-part slots, seed_slot the slot that placed the
   frame, status 0 used, 1 fewer than 2 taking-part slots, 3 dropped (fewer than 2 observations in front of the camera),
   4 in a solve that failed, 5 not connected to the world tag; d_result: one asl_map_result.  The host waits once, for the
   problem size (cameras, tags, observations), then enqueues the rest on `stream` and returns.  More than 1000 tags, or a
   world_id >= 0 that no used frame sees, is an error.  max_tags in [1, 256]; deterministic: the same input gives the same
   bytes.  tests/map_ref.py states the algorithm. */
int asl_map_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                          const double *dist, int n_dist, double tag_size, int world_id, int max_iters, void *d_map,
                          void *d_tag_std, void *d_poses, void *d_result, void *stream);
/* The same computation on host records, synchronous (the detector keeps the device copies and grows them on demand). */
int asl_map_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K,
                  const double *dist, int n_dist, double tag_size, int world_id, int max_iters, asl_map_tag *map,
                  double *tag_std, asl_cam_pose *poses, asl_map_result *result);

/* asl_map_frames_device with a robust (Huber) loss on every corner's pixel residual in the joint LM, for surveys where a
   corner slips or a slot carries another tag's corners (a mis-decoded id): under the squared loss one such slot in hundreds
   bends the whole map, and everything that later takes the map as exact with it.  The seed (gather, chain, reseed sweeps,
   gauge, flip test, behind-camera test) is the plain call's, with squared costs, bit for bit.  map_huber_px is the
   threshold every other layer calls huber_px: huber_px = k > 0, in pixels, on the raw residual r = (r0, r1) of a corner, s = |r|: s <= k costs s^2 with weight 1 (the plain term); s > k costs
   2 k s - k^2 with weight k / s; a corner at z <= 1e-9 costs 1e12, adds nothing and is never over, as before.  The corner
   adds weight J^T J and weight J^T r to the normal equations (iteratively reweighted Gauss-Newton, no second-order term of
   the loss).  The robust cost stands wherever the LM's squared one does: cost_seed and cost, every trial, the accept rule and
   the 1e-12 stop.  rms_px and rms_seed_px, per frame and in the result, are sqrt(sum of the corner costs / corners): the
   plain RMS whenever no corner is over the threshold.  Damping, the lambda schedule, statuses, max_iters and which frames,
   tags and observations are in the solve are those of the plain call; a frame's n_rejected keeps its meaning (nothing is
   removed: a bad observation is down-weighted).
   The result's n_soft is the number of observations in the solve with at least one corner of weight < 1 at the returned
   poses ("soft").  d_slot_weight (NULL: skipped): n_frames x max_tags doubles, for a slot in the solve the smallest of its
   four corner weights at the returned poses, in (0, 1]; 0 for every other slot, and for every slot, with n_soft 0, when the
   result's status is not 0.  The slots with a weight below 1 are the observations to look at.
   d_tag_std: the diagonal comes from the weighted undamped system at the solution, and the variance factor from the
   corners that are not over k: sigma^2 = sum of their s^2 / (2 n_in - 6 frames - 6 (tags - 1)), n_in their number (a corner
   at z <= 1e-9 is one of them, with its 1e12), 0 if that denominator is <= 0.  With cost / dof the linear tail of one swapped
   slot inflated every tag's std several times over; the inlier factor does not, and is biased slightly low by the truncation
   at k.
   The loss cannot repair a seed that leaves a tag in a wrong basin (the slot that seeds a frame carrying another tag's
   corners and PnP pose), nor a block too small to out-vote a bad slot (four frames of four tags); a k near the corner noise
   makes many slots soft (at 2 sigma about a third of them).  The linear tail may need more trials than the quadratic one:
   raise max_iters.  huber_px == 0 is the plain computation, run by the plain kernels: d_map, d_tag_std, d_poses and
   d_result are byte for byte what asl_map_frames_device writes, n_soft 0, the slot weights 1 for the slots in the solve.
   ASL_EINVAL, nothing written: whatever asl_map_frames_device refuses; huber_px < 0 or not finite.  The host waits once, as
   in the plain call; deterministic: the same input gives the same bytes.  tests/map_ref.py states the computation. */
int asl_map_robust_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                                 const double *dist, int n_dist, double tag_size, int world_id, double map_huber_px, int max_iters,
                                 void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight, void *stream);
/* The same computation on host records, synchronous; slot_weight may be NULL. */
int asl_map_robust_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K,
                         const double *dist, int n_dist, double tag_size, int world_id, double map_huber_px, int max_iters,
                         asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result, double *slot_weight);

/* Tag-map reconstruction from the frames of a camera rig: asl_map_robust_frames_device with the camera-major block
   d_obs[n_cams][n_frames][max_tags] and the asl_rig_camera table of asl_localize_rig_frames_device (n_cams records, complete
   when the call is made) in place of one camera's model.  A frame index is one instant for all cameras, the mountings are
   taken as exact and the rig has one tag_size.  Tags that no single camera ever sees together come into one map and one
   gauge through the rig's poses.  tests/map_ref.py states the computation:
   a view is a taking-part slot of one camera (flags & 1, 0 <= id < n_ids; a repeated id takes part once per camera, in that
   camera's first slot; the same id in two cameras of a frame is two views), in (frame, camera, slot) order.  A frame is used
   if its views hold >= 2 distinct ids.  The camera pose of a view is E_c (rig<-world): the seed's stages are the plain
   call's over views, a view's PnP pose going through its camera's mounting (the rig from a view: inv(E_c) T_obs inv(G); the
   tag from a view: inv(E_c W) T_obs), every corner costed by its own camera's model, areas in pixels as they are.  The
   behind-camera test drops a frame left with < 2 distinct tags among its views.  The joint LM has 6 unknowns per used frame
   (rig<-world) and per mapped tag but the world tag; all views of a (frame, tag) pair enter it.  rig_huber_px is the
   threshold every other layer calls huber_px, with asl_map_robust_frames_device's meaning, per view; 0: the squared loss.
   d_poses: T = world<-rig, n_tags the frame's views in the solve, n_rejected its other taking-part slots, seed_slot the
   seeding view as the frame's global slot camera * max_tags + slot; the result's n_obs, n_obs_dropped and n_soft count
   views, and the std's degrees of freedom are 8 views - 6 frames - 6 (tags - 1).  d_slot_weight (NULL: skipped):
   n_cams x n_frames x max_tags doubles, camera-major like the block.
   ASL_EINVAL, nothing written: whatever asl_map_robust_frames_device refuses; d_rig NULL; n_cams outside [1, 16];
   n_cams * max_tags > 256; a camera with n_dist not 0, 4 or 5, a non-finite K, dist or E, or an E whose rotation is not
   orthonormal to 1e-6 (the table is read back and checked before anything is enqueued).  Deterministic: the same input
   gives the same bytes. */
int asl_map_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids,
                              const void *d_rig, double tag_size, int world_id, double rig_huber_px, int max_iters, void *d_map,
                              void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight, void *stream);
/* The same computation on host records, synchronous; tag_std and slot_weight may be NULL. */
int asl_map_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids,
                      const asl_rig_camera *rig, double tag_size, int world_id, double rig_huber_px, int max_iters,
                      asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result, double *slot_weight);

/* Tag-map reconstruction for tags of different KNOWN sizes (large tags for far views, nested landing pads, two print
   sizes in one survey): asl_map_robust_frames_device / asl_map_rig_frames_device with the side of every tag id stated by
   the caller.  The poses are the unknowns; sizes are given, never estimated.  tag_sizes: n_ids float32 values, a HOST
   array in the device forms too, like K and dist, read before the call returns; NULL: no table, the call is then the
   robust / rig call to the byte.  The rule is the one of every solver that takes an asl_map_tag.size:
     tag_sizes[id] == 0            the tag has the call's tag_size: h = float32(tag_size / 2), as in the other map calls
     tag_sizes[id] > 0, finite     the tag's own side: h_id = (double)(tag_sizes[id] * 0.5f)
     negative or not finite        ASL_EINVAL naming the id, nothing written or enqueued (a map entry with such a size is
                                   an unmapped id to the localisation; here the table is the caller's own input)
   The sizes enter in two places.  Corners: every pass that forms a tag's corners (+-h, +-h, 0) uses that tag's h: the
   reseed sweeps of frames and of tags, the flip test with its pose-only LM, the behind-camera test, the joint LM's
   linearisation and costs (seed, every trial, final, per frame) and the robust call's weights.  Seeds: a record's PnP
   pose T was solved at the call's tag_size, so for a sized tag it has the right rotation and a translation short by
   tag_size / size; wherever T proposes a pose (the chain's frame and tag halves, the sweeps' candidates) a sized tag's
   translation is first multiplied by k = h_id / h, and the mirrored planar minimum is formed after that.  A tag without
   a size takes the unscaled path.  The flip test's mirror comes from the current map pose, not from T.  Everything else
   is the robust / rig call's: the slots that take part, the used frames, the world tag and the gauge, statuses, the
   lambda schedule and the stop rule, the Huber terms (sized_huber_px is the threshold every other layer calls huber_px;
   0: the squared loss), the std's degrees of freedom, determinism.
   d_map[id].size is tag_sizes[id] for every mapped id (0 where the table has 0) and unmapped ids stay all-zero, so the
   block goes to asl_localize_* / asl_smooth_* / asl_calibrate_* as it is, with the same tag_size.  Ids that no used frame
   sees may have any valid entry.  An all-zero table gives every output of the robust / rig call byte for byte; a table
   whose every entry equals a float32 tag_size gives the same bytes but for d_map[].size.
   tests/map_ref.py states the computation. */
int asl_map_sized_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                                const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id,
                                double sized_huber_px, int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result,
                                void *d_slot_weight, void *stream);
/* The same computation on host records, synchronous; tag_std and slot_weight may be NULL. */
int asl_map_sized_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K,
                        const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id,
                        double sized_huber_px, int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses,
                        asl_map_result *result, double *slot_weight);
/* The rig forms: asl_map_rig_frames_device / asl_map_rig_batch with the same table and rule; a tag has one size, whichever
   camera views it. */
int asl_map_rig_sized_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                    const void *d_rig, double tag_size, const float *tag_sizes, int world_id, double sized_huber_px,
                                    int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight,
                                    void *stream);
int asl_map_rig_sized_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids,
                            const asl_rig_camera *rig, double tag_size, const float *tag_sizes, int world_id, double sized_huber_px,
                            int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result,
                            double *slot_weight);

/* The joint covariance of a reconstructed map: asl_map_sized_frames_device / asl_map_rig_sized_frames_device (tag_sizes may
   be NULL, cov_huber_px is the threshold every other layer calls huber_px, 0: the squared loss) with, after d_slot_weight,
   the covariance BETWEEN the tags that d_tag_std gives only the diagonal of.  A per-tag std is not enough to carry the
   uncertainty of a map into a pose localised against it: the tags of a map share their frames, so their errors are
   correlated.  Sigma_map = s^2 S^-1, S the undamped reduced system over the tags at the returned solution (the weighted
   one under the Huber loss, with a rig's views folded: the system d_tag_std reads) and s^2 the variance factor of
   d_tag_std, restricted to the mapped tags other than the world tag; six parameters per tag, (omega, v) of a left update
   of world<-tag in the world frame, as d_tag_std.
   d_cov_slot: n_ids int32.  Entry i is the block k of id i in the matrix, blocks numbered in ascending id; -1 for the ids
   without a covariance: unmapped ids and the world tag.  d_map_cov: doubles, row-major with the leading dimension
   ld = 6 * cap_tags, cap_tags stated by the caller; rows and columns 6 k .. 6 k + 5 belong to block k.  Only the leading
   6 n_cov x 6 n_cov region is written, n_cov = result.n_tags - 1; it is symmetric to the bit, and the square roots of its
   diagonal are d_tag_std to rounding.  If the undamped system is not positive definite, or the result's status is not 0,
   every d_cov_slot entry is -1 and nothing of d_map_cov is written: the cases in which d_tag_std is all zero.  The gauge is
   the world tag, taken as exact; the covariance of the frame poses is not reported.
   Every other output is byte for byte that of the sized call on the same input (d_tag_std may be NULL).
   ASL_EINVAL, nothing written: whatever the sized call refuses; d_cov_slot or d_map_cov NULL; cap_tags < 1; more tags
   besides the world tag in the problem (the ids seen in used frames) than cap_tags, which is known after the call's one
   host wait and refused there, before anything else is enqueued.  The columns of L^-1 (S = L L^T) are kept in the
   detector's workspace, 8 (6 tags)^2 bytes.  Deterministic: the same input gives the same bytes.  tests/map_cov_ref.py
   states the computation. */
int asl_mapcov_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, int n_ids, const double *K,
                              const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id,
                              double cov_huber_px, int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result,
                              void *d_slot_weight, void *d_cov_slot, void *d_map_cov, int cap_tags, void *stream);
/* The same computation on host records, synchronous; tag_std and slot_weight may be NULL.  map_cov is cap_tags x cap_tags
   blocks of the caller's; the part outside the leading 6 n_cov x 6 n_cov region is left as it was. */
int asl_mapcov_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, int n_ids, const double *K,
                      const double *dist, int n_dist, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px,
                      int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result,
                      double *slot_weight, int32_t *cov_slot, double *map_cov, int cap_tags);
/* The rig forms: asl_map_rig_sized_frames_device / asl_map_rig_sized_batch with the same outputs. */
int asl_mapcov_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, int n_ids,
                                  const void *d_rig, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px,
                                  int max_iters, void *d_map, void *d_tag_std, void *d_poses, void *d_result, void *d_slot_weight,
                                  void *d_cov_slot, void *d_map_cov, int cap_tags, void *stream);
int asl_mapcov_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, int n_ids,
                          const asl_rig_camera *rig, double tag_size, const float *tag_sizes, int world_id, double cov_huber_px,
                          int max_iters, asl_map_tag *map, double *tag_std, asl_cam_pose *poses, asl_map_result *result,
                          double *slot_weight, int32_t *cov_slot, double *map_cov, int cap_tags);

/* ---- extending a map: the world<-tag pose of tags the map does not have, from frames whose camera poses are known
   (asl_localize_* against the tags the map does have, asl_smooth_*, or asl_map_*'s d_poses).  The dual of localisation:
   each unmapped tag is solved on its own from all its views with the cameras held fixed, one wavefront per tag.  The
   result is NOT the joint optimum of cameras and tags: the frame poses are taken as exact, exactly as localisation takes
   the map as exact, and their uncertainty is not propagated.  The known entries of the map are never moved, so the gauge
   and every pose the rest of a system relies on stay as they are. */
typedef struct {
    double rms_px;         /* final reprojection RMS (pixels per corner) over the views used */
    double rms_seed_px;    /* the same of the winning first candidate, over every view */
    int32_t n_views;       /* views in the final solve (status 2 and 3: the views found) */
    int32_t n_rejected;    /* views dropped by the gate */
    int32_t status;        /* 0 located, 1 not wanted, 2 fewer than min_views views, 3 no view with a PnP */
    int32_t seed_frame;    /* frame of the winning first candidate, -1 if none */
    int32_t seed_mirrored; /* 1: that candidate was the mirrored planar minimum */
    int32_t reserved;
} asl_tag_fit;             /* 40 bytes */

/* d_obs: n_frames x max_tags records of one camera; d_poses: n_frames asl_cam_pose (T = world<-camera); d_map: n_ids
   asl_map_tag, in and out; d_fit: n_ids asl_tag_fit; d_cov: n_ids asl_pose_cov or NULL.  Device pointers, asynchronous on
   `stream`, no host wait.
   Wanted: id i < n_ids whose entry has valid == 0 and a size that is >= 0 and finite.  size > 0 on such an entry is the
   tag's own known side, 0 means tag_size (the rule of asl_map_tag.size), so no separate table of sizes is needed.  Valid
   entries, and invalid ones with a negative or non-finite size, are not wanted: status 1.
   Views: frame f takes part if d_poses[f].status is 0 or 6 (the sequence solve's prior-only frame) and rows 0..2 of its T
   are finite; in such a frame the first slot with flags & 1 and id == i is the tag's view.  C_f = inv(T_f).  Fewer than
   min_views (>= 1) views: status 2.
   Cost: the 4 corners (+-h, +-h, 0) of every active view, project(C_f (G X_q)) - uv, G = world<-tag; a corner at
   z <= 1e-9 costs 1e12.  Seed: the <= 8 active views with flags & 2 of largest corner area (ties: the earlier view), in
   view order, each with G = inv(C_f) T_obs (a sized tag's PnP translation first times size / tag_size) and that pose's
   mirrored planar minimum formed in the camera frame; the strictly lowest total cost over all active views wins.  No such
   view, or every score NaN: status 3.  Refinement: Levenberg-Marquardt on the 6 parameters of G with localisation's fixed
   schedule.  max_view_rms_px > 0 is an outlier gate: while the active view of largest own 4-corner RMS exceeds it, that
   view is dropped (one at a time, at most 8, never the last) and the solve is seeded again, from the lowest-cost of the
   current pose and the candidates of the views still active, and refined; 0 turns the gate off.
   Output: a located tag's d_map[i].T is written and its valid set to 1, its size is kept; every other map entry keeps its
   bytes, so the block is the extended map and goes to asl_localize_* / asl_smooth_* / asl_calibrate_* as it is.  d_cov[i]:
   the covariance of world<-tag in the (r, d) convention above (the pose solved for itself, A = [I 0; -[p]x I]) over the
   views of the final solve, dof = 8 n_views - 6, sigma_px given or 0 to estimate it from the cost; status 1 for an id not
   located, 2 when J^T J is not positive definite.
   ASL_EINVAL, before anything is written or enqueued: a NULL argument other than d_cov, n_frames < 0, max_tags outside
   [1, 256], n_ids < 1, a bad camera, a negative or non-finite gate, min_views < 1, sigma_px < 0 or non-finite.
   n_frames == 0 is ASL_OK: every wanted id gets status 2.  Deterministic: the same input gives the same bytes.
   tests/locate_ref.py states the computation. */
int asl_locate_tags_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_poses,
                                  void *d_map, int n_ids, const double *K, const double *dist, int n_dist, double tag_size,
                                  double max_view_rms_px, int min_views, double sigma_px, void *d_fit, void *d_cov, void *stream);
/* The same computation on host records, synchronous; map is read and written in place, cov may be NULL. */
int asl_locate_tags_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_cam_pose *poses,
                          asl_map_tag *map, int n_ids, const double *K, const double *dist, int n_dist, double tag_size,
                          double max_view_rms_px, int min_views, double sigma_px, asl_tag_fit *fit, asl_pose_cov *cov);

/* The rig form: asl_locate_tags_* with the camera-major block d_obs[n_cams][n_frames][max_tags] and the camera table
   d_rig (n_cams asl_rig_camera, complete when the call is made) of asl_localize_rig_* in place of K, dist, n_dist.  A tag
   that only a camera without a mapped tag in view sees is located through the rig's pose; a tag two cameras see at one
   instant is solved from both views.
   Poses: d_poses holds n_frames records with T = world<-rig, what asl_localize_rig_*, asl_smooth_rig_* and asl_map_rig_*
   write.  A frame takes part under the rule above (status 0 or 6, rows 0..2 finite).
   Views: in a frame that takes part each camera c = 0..n_cams-1 gives at most one view of id i, its first slot with
   flags & 1 and id == i; the same id in two cameras of a frame is two views (asl_map_rig_*'s rule).  View order is
   (frame, camera).  The camera of a view is C = E_c inv(T_f) = (Re R, Re t + te) with inv(T_f) = (R, t) formed as above,
   and every view is projected through its own camera's model.  min_views counts views: one frame seen by two cameras
   satisfies min_views = 2.
   Seed, refinement, gate with re-seeding, fit record and covariance are those above over this view list.  The seeds are
   the <= 8 active views with flags & 2 of largest corner area; areas are pixels as they are, so cameras of different
   focal length are not put on one scale (asl_localize_rig_*'s rule); ties go to the earlier view.  A candidate is
   G = inv(C) T_obs, plain before mirrored, a sized tag's translation first times size / tag_size.  The gate drops single
   views: a spoiled view in one camera leaves the other cameras' views of that frame in.  seed_frame is the frame of the
   winning first view; reserved stays 0.  The covariance has dof = 8 n_views - 6; the mountings and the frame poses are
   taken as exact.
   ASL_EINVAL, before anything is written or enqueued: whatever asl_locate_tags_* refuses, d_rig NULL, n_cams outside
   [1, 16], n_cams * max_tags > 256, n_cams * n_frames * max_tags >= 2^31, or a table with a bad n_dist, a non-finite
   entry or an E whose rotation part is not a rotation; the device form reads the table back and checks it first.
   n_frames == 0 is ASL_OK: every wanted id gets status 2.  Deterministic: the same input gives the same bytes.  A rig of
   one camera with E = I is asl_locate_tags_* with that camera.  tests/locate_rig_ref.py states the computation. */
int asl_locate_tags_rig_frames_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags,
                                      const void *d_poses, void *d_map, int n_ids, const void *d_rig, double tag_size,
                                      double max_view_rms_px, int min_views, double sigma_px, void *d_fit, void *d_cov,
                                      void *stream);
/* The same computation on host records, synchronous; map is read and written in place, cov may be NULL. */
int asl_locate_tags_rig_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags,
                              const asl_cam_pose *poses, asl_map_tag *map, int n_ids, const asl_rig_camera *rig,
                              double tag_size, double max_view_rms_px, int min_views, double sigma_px, asl_tag_fit *fit,
                              asl_pose_cov *cov);

/* ---- sequence localisation: the camera poses of one camera's consecutive frames against a fixed map, solved together
   under a random-walk motion prior, so that EVERY frame gets a pose: frames without a mapped tag are carried by their
   neighbours, a single-tag frame cannot end in its mirrored planar minimum alone, and corner noise is averaged. */
typedef struct {
    double cost_seed, cost;        /* the objective below after the seed chain / at the end */
    double rms_px, rms_seed_px;    /* pixel residuals alone, per corner, over all frames: at the end / after the chain */
    int32_t n_frames_data;         /* frames with a taking-part slot */
    int32_t n_filled;              /* frames without a seed pose, started from a neighbour's */
    int32_t n_flipped;             /* frames where the chain chose the mirrored candidate */
    int32_t iterations;            /* LM trials run */
    int32_t status;                /* 0 ok, 1 no frame with a seed pose (nothing solved), 2 never positive definite,
                                      3 non-finite cost after the chain, 4 (asl_smooth_timed_sequences_*) the sequence's
                                      times are bad: one not finite, or two consecutive ones that do not increase */
    int32_t n_soft;                /* asl_smooth_robust_sequences_*: taking-part slots, over all frames, with a corner over the
                                      threshold at the returned poses (the frames' n_rejected summed); 0 from the plain calls */
    int32_t reserved[2];
} asl_smooth_result;               /* 64 bytes */

/* Smooth d_obs (n_frames x max_tags records of consecutive frames, as asl_pack_observations_device writes them) against
   d_map (n_ids asl_map_tag; tag_size is the size of the entries whose size is 0) from d_seed (n_frames asl_cam_pose, what asl_localize_frames_device wrote for the same obs, map
   and camera; status 0: the frame has a pose); device pointers, everything enqueued on `stream`, no host wait (the detector
   owns the work buffers: the first call at a larger n_frames allocates, which synchronises the device).  Unknowns:
   camera<-world (R_f, t_f) of every frame, left update as the localisation.  Minimised:
   sum_f |r_f|^2 / sigma_px^2 + sum_f |(Log(R_D) / sigma_rot, t_D / sigma_trans)|^2, r_f the localisation's residuals of
   frame f (slots with flags & 1 and a mapped id, the camera model of asl_solve_pnp_batch, a corner at z <= 1e-9 costs 1e12,
   no gate), R_D = R_{f+1} R_f^T, t_D = t_{f+1} - R_D t_f; sigma_rot in radians, sigma_trans in scene units, per frame step.
   Seed chain: each posed frame has its seed pose A and, with exactly one taking-part slot, the mirrored planar minimum B
   through that slot's map tag; a two-state dynamic programme over the posed frames picks one per frame (data cost plus
   motion cost, divided by the gap in frames; ties to A); a frame without a seed pose starts from the nearest earlier posed
   frame's (the leading ones from the first).  Then Levenberg-Marquardt on all frames: block-tridiagonal normal matrix,
   motion Jacobians to first order in the relative rotation, block Cholesky forward and back over the frames, lambda0 1e-3,
   x10 rejected or not positive definite / x0.1 accepted, at most max_iters trials (in [1, 100]; all enqueued, the ones after
   the stop return at once), stop on an accepted trial of relative decrease below 1e-12.
   d_out: n_frames asl_cam_pose, T world<-camera, rms_px / rms_seed_px the frame's own corner RMS at the end / after the
   chain, n_tags its taking-part slots, n_rejected 0, seed_slot the seed's (+256 if the chain chose B, -1 for a frame without
   a seed pose), status 0 solved with data, 6 solved and carried by the motion prior alone, 4 in a solve that failed (result
   status 2 or 3; T is the chain's), 1 nothing to solve (T the identity).  d_result: one asl_smooth_result.
   ASL_EINVAL, nothing written: a NULL pointer; n_frames outside [1, 65535]; max_tags outside [1, 256]; n_dist not 0, 4 or 5,
   or n_dist > 0 with dist NULL; a non-finite K, tag_size or sigma; a sigma <= 0; max_iters outside [1, 100]; d_out
   overlapping d_seed.  One sequence per call (several: asl_smooth_sequences_device), one frame step one unit of time
   (frame times: asl_smooth_timed_sequences_device).  Deterministic:
   the same input gives the same bytes.  tests/smooth_ref.py states the algorithm. */
int asl_smooth_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                             const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed, double sigma_px,
                             double sigma_rot, double sigma_trans, int max_iters, void *d_out, void *d_result, void *stream);
/* The same computation on host records, synchronous (the detector keeps the device copies and grows them on demand).
   seed == NULL: the per-frame localisation (asl_localize_frames_device, max_tag_rms_px 0) runs first and seeds it. */
int asl_smooth_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                     const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed, double sigma_px,
                     double sigma_rot, double sigma_trans, int max_iters, asl_cam_pose *out, asl_smooth_result *result);

/* asl_smooth_frames_device with the covariance of every frame's world<-camera pose: d_out and d_result receive exactly what
   the plain call writes, byte for byte; d_cov one asl_pose_cov per frame, in the convention above.  The objective is already
   whitened by sigma_px, sigma_rot and sigma_trans, so the covariance of the stacked left updates (w, v) of all frames is
   A^-1, A the undamped block-tridiagonal normal matrix at the returned poses, with no sigma^2 factor and no estimate from
   the residuals; a frame's record is its own diagonal block Sigma_ff of A^-1 (the marginal: the other frames are not held
   fixed), mapped as C_f = diag(-R_f^T, -R_f^T) Sigma_ff diag(-R_f^T, -R_f^T)^T.  Block Cholesky forward over the frames,
   then back: Sigma_{n-1} = L^-T L^-1, Sigma_f = L_f^-T (I + M_f^T Sigma_{f+1} M_f) L_f^-1.  A frame carried by the prior
   alone (status 6) has the covariance the prior leaves it: it grows with the distance to the nearest frames with data.
   sigma_px: the given one.  dof: 8 (taking-part slots of all frames) - 6, the same in every record (0 with status 1).
   status: 0 ok; 1 the solve has none (result status != 0: frame status 1 or 4); 2 A is not positive definite (a pivot not
   above 1e-13 of its diagonal entry: e.g. posed frames without any taking-part slot, where the prior alone leaves six
   directions free) -- in every record, because the inverse is global.  cov is all zero with status != 0.
   ASL_EINVAL, nothing written: whatever the plain call refuses; a NULL d_cov; d_cov overlapping d_out or d_seed.
   Deterministic: the same input gives the same bytes.  tests/smooth_cov_ref.py states the computation. */
int asl_smooth_cov_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                 const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed, double sigma_px,
                                 double sigma_rot, double sigma_trans, int max_iters, void *d_out, void *d_result, void *d_cov,
                                 void *stream);
/* The same computation on host records, synchronous; seed as asl_smooth_batch. */
int asl_smooth_cov_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                         const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed, double sigma_px,
                         double sigma_rot, double sigma_trans, int max_iters, asl_cam_pose *out, asl_smooth_result *result,
                         asl_pose_cov *cov);

/* Several sequences in one call, solved side by side: sequence k is the frames [seq_start[k], seq_start[k + 1]) of d_obs,
   d_seed, d_out and d_cov (different cameras, recordings, or the pieces of a recording cut where the camera was off).
   Sequence k's d_out records, its d_cov records and d_results[k] are, byte for byte, what asl_smooth_cov_frames_device
   (d_cov NULL: asl_smooth_frames_device) writes for those frames alone with the same arguments; d_out and d_results do not
   depend on whether d_cov is given.  No term links two sequences: no motion block across a boundary, no seed carried over,
   and each has its own lambda, stop, failed trials, result status, covariance status and dof -- one that stops early, fails
   (status 1, 2, 3) or has no covariance changes nothing in another.  The map, the camera, the sigmas, max_iters and max_tags
   are the call's.  The serial chains over the frames run one wavefront per sequence, side by side, so the chains' share of
   the time is that of the slowest sequence (frames x trials), not the sum (DESIGN.md 7g has the measurements).  d_results: n_seq asl_smooth_result.  d_cov: NULL, or n_frames asl_pose_cov.
   seq_start: a HOST array of n_seq + 1 offsets, as K and dist are host arrays; it is read before the call returns (the
   caller may overwrite it then) and reaches the device in stream order, so calls enqueued back to back each see their own.
   Nothing waits; the first call at a larger n_frames or n_seq grows the work buffers, which synchronises.
   ASL_EINVAL, nothing written: whatever the single-sequence calls refuse, except that n_frames may be in [1, 1048576];
   seq_start NULL; n_seq outside [1, 65535]; seq_start[0] != 0; seq_start[n_seq] != n_frames; a sequence of fewer than 1 or
   more than 65535 frames (offsets that do not strictly increase).  Deterministic: the same input gives the same bytes. */
int asl_smooth_sequences_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                int max_iters, void *d_out, void *d_results, void *d_cov, void *stream);
/* The same computation on host records, synchronous; seed == NULL: the per-frame localisation of all frames runs first, as
   in asl_smooth_batch.  results: n_seq records.  cov: NULL, or n_frames records. */
int asl_smooth_sequences_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                               const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                               const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                               int max_iters, asl_cam_pose *out, asl_smooth_result *results, asl_pose_cov *cov);

/* asl_smooth_sequences_device with a robust (Huber) loss on every corner's pixel residual, for footage where a corner slips
   or a slot carries another tag's corners: the squared loss lets one such slot bend its frame and, through the prior, its
   neighbours.  huber_px = k > 0, in pixels, on the raw residual r = (r0, r1) of a corner (before sigma_px), s = |r|:
   s <= k costs s^2 with weight 1 (the plain term); s > k costs 2 k s - k^2 with weight k / s; a corner at z <= 1e-9 costs 1e12
   and adds nothing, as before.  The frame's data cost is the sum of these, divided by sigma_px^2 where |r_f|^2 is in the plain
   objective; the corner adds weight J^T J and weight J^T r to the normal equations (iteratively reweighted Gauss-Newton, no
   second-order term of the loss).  The robust cost stands wherever the squared one does: the candidates of the seed chain,
   the cost after the chain, every trial and the accept rule, cost_seed and cost.  rms_px and rms_seed_px, per frame and in
   the result, are sqrt(sum of the corner costs / corners): the plain RMS whenever no corner is over the threshold.
   A frame's n_rejected is the number of its taking-part slots with at least one corner of weight < 1 at the returned poses
   ("soft" slots: down-weighted, not removed); the result's n_soft is their sum over the sequence's frames.  The motion
   prior, the linear solve, the LM schedule, the stop rule and the fill of unposed frames are those of the plain call, and
   n_seq = 1 is the single sequence.
   d_cov (NULL: none): as asl_smooth_cov_frames_device, A built from the weighted normal equations at the returned poses, so
   a down-weighted corner contributes k / s of its information; d_out and d_results do not depend on whether it is given.
   A frame whose only tag carries the outlier has nothing to be corrected by except its neighbours through the prior.  The
   linear tail of the loss needs more trials than the quadratic one (a corrupted 40-frame scene used all 30 it was given
   where the clean one stopped after 5): raise max_iters.  huber_px == 0 is the plain computation: d_out, d_results and d_cov are byte for byte what
   asl_smooth_sequences_device writes, n_soft 0.
   ASL_EINVAL, nothing written: whatever asl_smooth_sequences_device refuses; huber_px < 0 or not finite.  Nothing waits;
   deterministic: the same input gives the same bytes.  tests/smooth_ref.py states the computation (huber_px > 0). */
int asl_smooth_robust_sequences_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                       const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                       const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                       double huber_px, int max_iters, void *d_out, void *d_results, void *d_cov, void *stream);
/* The same computation on host records, synchronous; seed == NULL: the per-frame localisation of all frames runs first, as
   in asl_smooth_sequences_batch. */
int asl_smooth_robust_sequences_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                      const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                                      const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                      double huber_px, int max_iters, asl_cam_pose *out, asl_smooth_result *results, asl_pose_cov *cov);

/* asl_smooth_robust_sequences_device with a time for every frame, for footage whose frames are not evenly spaced: dropped
   frames, a camera pause, a variable frame rate.  d_times: n_frames doubles on the device, any unit, read in stream order
   (no host wait); sigma_rot and sigma_trans are then the random walk's sigmas per unit of that time.  The pair (f, f + 1) of
   a sequence, dt = d_times[f + 1] - d_times[f], has the motion residual (Log(R_D) w_rot, t_D w_trans) with
   w_rot = (1 / sigma_rot) (1 / sqrt(dt)) and w_trans = (1 / sigma_trans) (1 / sqrt(dt)): its cost is the plain one divided by
   dt, which is what marginalising dt - 1 evenly spaced frames without data out of the plain problem leaves.  The seed chain
   divides the motion cost between a posed frame and its posed predecessor p by d_times[f] - d_times[p] where the plain call
   divides by f - p.  Nothing else changes: the corner costs (huber as huber_px of the robust call, 0: squared), the linear
   solve, the LM schedule, the fill, the outputs; d_cov is the inverse of the timed matrix.  Times of different sequences
   are unrelated: no term links two sequences, so a later sequence may start at an earlier time.
   d_times NULL is frame f at time f: d_out, d_results and d_cov are byte for byte what asl_smooth_robust_sequences_device
   writes; so are they for times of unit spacing, d_times[f] = c + f with exact differences.
   Bad times are found on the device, per sequence: a time that is not finite, or a dt <= 0 inside the sequence (a sequence
   of one frame needs only a finite time).  That sequence's result has status 4 and is otherwise the result of status 1, its
   frames have the records of status 1 (T the identity, seed_slot -1), its d_cov records status 1; the other sequences of
   the call are what they are without it, so a sequence of a batch stays byte for byte what the call alone returns.
   ASL_EINVAL, nothing written: whatever asl_smooth_robust_sequences_device refuses; d_times overlapping d_out or d_cov.
   Nothing waits; deterministic: the same input gives the same bytes.  tests/smooth_ref.py states the computation (times). */
int asl_smooth_timed_sequences_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                      const double *K, const double *dist, int n_dist, double tag_size, const void *d_seed,
                                      const double *d_times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                      double sigma_trans, double huber, int max_iters, void *d_out, void *d_results, void *d_cov,
                                      void *stream);
/* The same computation on host records, synchronous; times: a host array of n_frames doubles or NULL, copied to the device
   as the seed is; bad times give status 4 here too, not ASL_EINVAL.  seed == NULL as in asl_smooth_sequences_batch. */
int asl_smooth_timed_sequences_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                                     const double *K, const double *dist, int n_dist, double tag_size, const asl_cam_pose *seed,
                                     const double *times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                     double sigma_trans, double huber, int max_iters, asl_cam_pose *out, asl_smooth_result *results,
                                     asl_pose_cov *cov);

/* Sequence localisation for a rig: asl_smooth_timed_sequences_device over the cameras of asl_localize_rig_frames_device.
   One pose rig<-world per frame of the rig's consecutive frames, minimising the reprojection error of all mapped corners of
   all cameras (/ sigma_px^2; a corner X of camera c contributes project_c(E_c (rig<-world) X) - pixel, through a Huber loss
   of rig_huber_px pixels as in asl_smooth_robust_sequences_device, 0: squared) plus the random-walk motion prior between
   consecutive rig poses.  Everything between frames -- the seed chain's dynamic programme, the fill of unposed frames, the
   block-tridiagonal solve, the LM schedule, the stop rule, several sequences side by side, the frame times and the
   covariance -- is that of the single-camera calls.
   d_obs: n_cams x n_frames x max_tags records, camera-major as for asl_localize_rig_frames_device, n_frames the frames of
   the whole call (all sequences end to end); a frame's records are its global slots g = c * max_tags + s.  d_rig: n_cams
   asl_rig_camera in device memory, read back and checked before anything is enqueued (the one synchronous step), so it
   must be complete when the call is made.  tag_size is one value for the rig.  d_seed: one asl_cam_pose per frame, what
   asl_localize_rig_frames_device wrote for the same block (T = world<-rig; status 0: posed).  d_frame_times: NULL (frame f
   is at time f), or n_frames doubles on the device as d_times of asl_smooth_timed_sequences_device.  seq_start, n_seq: as
   asl_smooth_sequences_device; one sequence is n_seq = 1 with seq_start = {0, n_frames}.
   Seed chain: candidate A is the seed's rig<-world.  B exists for a frame with exactly one taking-part global slot over
   all cameras and goes through that slot's camera c: camera_c<-tag = E_c A map[id], its mirrored planar minimum, taken back
   through inv(map[id]) and inv(E_c).
   d_out: one asl_cam_pose per frame with T = world<-rig; n_tags counts taking-part global slots, n_rejected the soft ones,
   rms_px / rms_seed_px are over the corners of all cameras, seed_slot is the seed's global slot (+256 where the chain chose
   B, -1 for a filled frame), status as in asl_smooth_frames_device (0 data, 6 no mapped tag in any camera, carried by the
   prior, 4 failed solve, 1 nothing to solve).  d_results: n_seq asl_smooth_result.  d_cov: NULL, or one asl_pose_cov per
   frame of the world<-rig pose, as asl_smooth_cov_frames_device; the mountings and the map are taken as exact.  A rig of one
   camera with E = identity solves the single-camera problem (the same numbers to rounding, not the same bytes).
   ASL_EINVAL, nothing written or enqueued: whatever asl_smooth_timed_sequences_device refuses of the arguments both have;
   d_rig NULL; n_cams outside [1, 16]; n_cams * max_tags > 256; a camera with n_dist not 0 / 4 / 5, a non-finite K or E or
   an E whose rotation part is not orthonormal to 1e-6.  Deterministic: the same input gives the same bytes.
   tests/smooth_ref.py states the computation (smooth_rig). */
int asl_smooth_rig_sequences_device(asl_detector *det, const void *d_obs, int n_cams, int n_frames, int max_tags, const void *d_map,
                                    int n_ids, const void *d_rig, double tag_size, const void *d_seed, const double *d_frame_times,
                                    const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot, double sigma_trans,
                                    double rig_huber_px, int max_iters, void *d_out, void *d_results, void *d_cov, void *stream);
/* The same computation on host records, synchronous; frame_times, seed and cov may be NULL.  seed == NULL: the rig
   localisation of all frames (asl_localize_rig_batch, max_tag_rms_px 0) runs first, as asl_smooth_batch does for one camera. */
int asl_smooth_rig_sequences_batch(asl_detector *det, const asl_obs *obs, int n_cams, int n_frames, int max_tags, const asl_map_tag *map,
                                   int n_ids, const asl_rig_camera *rig, double tag_size, const asl_cam_pose *seed,
                                   const double *frame_times, const int32_t *seq_start, int n_seq, double sigma_px, double sigma_rot,
                                   double sigma_trans, double rig_huber_px, int max_iters, asl_cam_pose *out, asl_smooth_result *results,
                                   asl_pose_cov *cov);

/* ---- before the detector: the image-formation step on the device (reference src/simulation/renderer.py:197-274:
   purple clear colour, one GL_LINEAR-textured quad per tag, BGR read-back).  One plane per visible tag and frame, in
   painter's order (far to near); a plane with tex < 0 ends a frame's list. */
typedef struct {
    double Hi[9];     /* row-major 3x3: pixel centre (x+0.5, y+0.5, 1) -> tag plane (X, Y, w); with lens coefficients it maps
                         UNDISTORTED NORMALISED image coordinates instead */
    int32_t bbox[4];  /* x0, x1, y0, y1: pixels outside [x0,x1) x [y0,y1) cannot hit the tag */
    int32_t tex;      /* index into d_textures */
    int32_t pad;
} asl_render_plane;   /* 96 bytes */

/* Renders n_frames BGR frames of w x h pixels into device memory.  d_planes: n_frames x max_planes asl_render_plane
   (device), far to near, a record with tex < 0 ends a frame's list;
   d_textures: n_tex gray textures of tw x th bytes, rows top to bottom (device); half = half the side of the textured quad
   in scene units.  K (9 doubles) and dist (n_dist = 4 or 5) are host pointers and only needed for a camera with lens
   distortion (the reference's webcam caller, src/detection/video_detection.py:209-296); pass K = NULL for the
   simulator's pinhole. */
int asl_render_frames_device(asl_detector *det, void *d_frames, int n_frames, int w, int h, int stride, size_t frame_pitch,
                             const void *d_planes, int max_planes, const void *d_textures, int tw, int th, double half,
                             const double *K, const double *dist, int n_dist, void *stream);

/* Lens rectification, the step between calibration and detection (what cv2.undistort / remap do for upstream's users):
   n_frames gray or BGR frames of a camera with a lens (K 9 doubles row-major, dist n_dist = 0, 4 or 5 coefficients
   k1 k2 p1 p2 [k3], as asl_solve_pnp_batch; host pointers) in, the GRAY frames of w_out x h_out pixels an ideal pinhole
   K_new (9 doubles, NULL = K) would have delivered out; device pointers, frame i at d_src + i*frame_pitch and
   d_dst + i*frame_pitch_out, asynchronous on `stream`.  Output pixel (x, y): xn = (x + 0.5 - cx') / fx',
   yn = (y + 0.5 - cy') / fy' under K_new; the forward Brown-Conrady model, closed form (r2 = xn^2 + yn^2,
   rad = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = xn rad + 2 p1 xn yn + p2 (r2 + 2 xn^2), yd = yn rad + p1 (r2 + 2 yn^2) + 2 p2 xn yn);
   u = fx xd + cx, v = fy yd + cy under K.  A sample outside the source (not 0 <= u < w and 0 <= v < h) gives `fill`;
   otherwise the source is sampled bilinearly at (u, v), texel centres at +0.5, the four taps clamped to the edge, a BGR
   tap first turned into gray with the detector's formula ((3735 B + 19235 G + 9798 R + 16384) >> 15), and the result is
   floor(o + 0.5).  All in float64: the frames are byte-identical to tests/rectify_ref.py, and n_dist = 0 with
   K_new = NULL at the source's size is the detector's gray conversion, exactly.  Detections on the result are in
   rectified pixels: their camera is K_new with no distortion.  The detector supplies the device only; no batch state is
   touched, so the call is legal between submit and collect.
   ASL_EINVAL, nothing written: channels not 1 or 3; a size that is not positive (or above 16384); a stride or pitch
   smaller than a row or frame; n_dist not 0, 4 or 5, or n_dist > 0 with dist NULL; a non-finite entry of K, K_new or
   dist; fx or fy <= 0 in either matrix; fill outside 0..255; source and destination ranges that overlap. */
int asl_rectify_frames_device(asl_detector *det, const void *d_src, int n_frames, int channels, int w, int h,
                              int stride, size_t frame_pitch, void *d_dst, int w_out, int h_out, int stride_out,
                              size_t frame_pitch_out, const double *K, const double *dist, int n_dist,
                              const double *K_new /* 9, or NULL = K */, int fill, void *stream);
/* The same for one host image, synchronous: the cv2.undistort of one frame (the detector keeps the device copies and
   grows them on demand).  Only the w_out bytes of each of the h_out destination rows are written. */
int asl_rectify_u8(asl_detector *det, const uint8_t *src, int channels, int w, int h, int stride,
                   uint8_t *dst, int w_out, int h_out, int stride_out, const double *K, const double *dist,
                   int n_dist, const double *K_new, int fill);

/* Rectification into rotated pinhole views: the way in for a lens no single pinhole holds, a 150-200 degree fisheye.  The
   frame is rectified into n_views pinholes (K, R), each turned against the source camera (left, front and right at 90
   degrees each, say); those are rigidly mounted pinhole cameras with exactly known mountings, camera<-rig = [R^T | 0] in
   the source camera's frame, and every asl_*_rig_* solver takes their observations as they are.
   Output pixel (x, y) of view (K', R), R = source camera <- view, 9 doubles row-major:
     the view ray dv = ((x + 0.5 - cx') / fx', (y + 0.5 - cy') / fy', 1) and the source ray (X, Y, Z) = R dv, each
     component r0*dv0 + r1*dv1 + r2*dv2 from left to right; then the lens (K, dist, lens_model) of the source:
     ASL_LENS_BROWN, n_dist 0, 4 or 5 (k1 k2 p1 p2 [k3]): Z <= 0 gives `fill`; else xn = X / Z, yn = Y / Z and the closed
       form of asl_rectify_frames_device.  With one view and R the identity this is asl_rectify_frames_device, byte for byte.
     ASL_LENS_FISHEYE, n_dist 0 or 4 (k1 k2 k3 k4): the model of cv2.fisheye, carried past 90 degrees by the two-argument
       arctangent: r = sqrt(X*X + Y*Y), theta = atan2(r, Z) in [0, pi]; theta > theta_max gives `fill`; t2 = theta*theta,
       theta_d = theta (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))); s = theta_d / r (r == 0: s = 0);
       u = fx (s X) + cx, v = fy (s Y) + cy.  A ray behind the camera (Z < 0) is an ordinary ray of this model.
     then the outside test, the bilinear sample, the gray conversion and the rounding of asl_rectify_frames_device.
   All in float64, and the arctangent is an argument reduction and a polynomial written out in the kernel
   (tests/rectify_views_ref.py: atan2_pos), not the device library's, so the frames are byte-identical to that statement.
   theta_max: 0 means pi; otherwise in (0, pi]; cut it where the lens's image circle ends.  Ignored for ASL_LENS_BROWN.
   Layout: view v of frame i at d_dst + (v*n_frames + i)*frame_pitch_out -- view-major, so that the frames of one view are
   a contiguous batch for asl_submit_batch_device, and the order of the rig observation block (camera-major).  `views` is
   a host pointer, read before the call returns; asynchronous on `stream`.  Legal between submit and collect.
   Views that overlap show a tag twice, from the same source pixels: the rig solvers take both slots, which are not
   independent, so a covariance that counts both is somewhat optimistic.  Views that abut avoid it.
   ASL_EINVAL, nothing written: everything asl_rectify_frames_device refuses (the destination range being that of all
   views); lens_model not 0 or 1; ASL_LENS_FISHEYE with n_dist not 0 or 4; n_views outside 1..ASL_MAX_VIEWS or views
   NULL; a view whose K is not finite or has fx or fy <= 0; a view whose R is not finite or not a rotation
   (max |R R^T - I| > 1e-6 or det <= 0); theta_max not finite or outside [0, pi]. */
#define ASL_LENS_BROWN 0
#define ASL_LENS_FISHEYE 1
#define ASL_MAX_VIEWS 16
typedef struct { double K[9]; double R[9]; } asl_rectify_view;   /* 144 bytes; R = source<-view, row-major */
int asl_rectify_views_device(asl_detector *det, const void *d_src, int n_frames, int channels, int w, int h,
                             int stride, size_t frame_pitch, void *d_dst, int w_out, int h_out, int stride_out,
                             size_t frame_pitch_out, const double *K, const double *dist, int n_dist, int lens_model,
                             const asl_rectify_view *views /* host */, int n_views, double theta_max, int fill,
                             void *stream);
/* The same for one host image, synchronous: view v at dst + v*view_pitch_out (at least stride_out*h_out).  Only the
   w_out bytes of each of the h_out rows of each view are written. */
int asl_rectify_views_u8(asl_detector *det, const uint8_t *src, int channels, int w, int h, int stride,
                         uint8_t *dst, int w_out, int h_out, int stride_out, size_t view_pitch_out, const double *K,
                         const double *dist, int n_dist, int lens_model, const asl_rectify_view *views, int n_views,
                         double theta_max, int fill);

/* ---- camera calibration with the lens named: asl_calibrate_frames_device / asl_calibrate_batch with lens_model before
   n_dist, the same asl_calib_result (216 bytes), per-frame records, statuses, schedule and uncertainty.
   ASL_LENS_BROWN: those two calls, byte for byte.
   ASL_LENS_FISHEYE: the cv2.fisheye model as asl_rectify_views_device states it (the same arctangent), n_dist 0 (pure
     equidistant) or 4: dist[0..3] = k1 k2 k3 k4 and std[4..7] their standard deviations, dist[4] and std[8] are 0.  What a
     150-200 degree lens needs before asl_rectify_views_device can serve it: calibrate from the RAW frames' corners, then
     rectify with the K and dist this returns.  A corner past 90 degrees off axis is an ordinary corner (none is "behind the
     camera"; a corner costs 1e12 only in the camera centre itself, |P| <= 1e-9), and on the axis projection and Jacobian
     are their finite limits.  Neither Zhang's closed form nor the planar pose of a quad holds under this lens, so without
     K_init the principal point starts at the image centre and the focal length comes from a ladder of 13 rungs
     f_j = max(width, height) / pi * 2^((j - 4) / 4), j = 0..12: at each rung every taking-part frame is seeded under the
     equidistant (f_j, f_j, centre) -- of the slots whose four corners all unproject to within 1.3 rad of the axis, the <= 8
     of largest area; each slot's corner rays as pinhole coordinates give its planar pose and the mirrored minimum, scored
     over all the frame's corners under the fisheye; the strictly lowest is refined by the pose-only LM -- and the rung's
     score is the sum of its frames' seed costs plus 1e12 per frame without a candidate; the lowest score wins (ties: the
     lower rung); status 2 if no frame has a candidate there.  With K_init the ladder is skipped and the frames are seeded
     under K_init.  A frame without a candidate at K0 gets status 3.  rms_init_px is the rms after the seed under K0 with
     k = 0.  The joint LM's columns are (w, v, fx, fy, cx, cy, k1, k2, k3, k4).  One submission, no host wait,
     deterministic.  tests/calib_fisheye_ref.py states the algorithm.
   ASL_EINVAL, nothing written: everything asl_calibrate_frames_device refuses; lens_model not 0 or 1; ASL_LENS_FISHEYE
   with n_dist not 0 or 4 or with ASL_CALIB_ZERO_TANGENT_DIST. */
int asl_calibrate_lens_frames_device(asl_detector *det, const void *d_obs, int n_frames, int max_tags, const void *d_map, int n_ids,
                                     double tag_size, int width, int height, const double *K_init /* 9 or NULL */, int lens_model,
                                     int n_dist, int flags, int max_iters, void *d_result, void *d_poses, void *stream);
int asl_calibrate_lens_batch(asl_detector *det, const asl_obs *obs, int n_frames, int max_tags, const asl_map_tag *map, int n_ids,
                             double tag_size, int width, int height, const double *K_init, int lens_model, int n_dist, int flags,
                             int max_iters, asl_calib_result *result, asl_cam_pose *poses);

/* ---- introspection and diagnostics.  asl_debug_fetch, asl_stage_times and the counters (item 5) describe the LAST batch
   the detector ran.  asl_detect_batch_u8 and asl_detect_batch_pose_u8 run a call of 128 frames or more as consecutive
   batches of 64 frames, so after such a call that is the call's last chunk (frames 128..149 of a 150-frame call), not the
   whole call.  asl_debug_fetch, asl_debug_refit, asl_debug_dedup, asl_debug_gn_cholesky, asl_debug_gn_step, asl_debug_division_check and
   asl_debug_phase_cycles are told the room
   they may write into and return ASL_EINVAL, writing nothing, when it is too small; asl_stage_times fills at most max_n. */

/* Copy an intermediate buffer of the last batch to host, for the parity tests.
   what: 0 = decimated gray as the threshold read it: blurred / sharpened under quad_sigma (u8, B*sh*sw)
         1 = threshold image (u8, B*sh*sw)
         2 = component labels (u32, B*sh*sw)  3 = component sizes by label (u32, B*sh*sw)
         4 = candidate quads (asl_debug_quad, count via *n_items)
         5 = stage counters (int64[18]: frames, sw, sh, clusters, points, quads, detections, ..., tiles of the two dense launches)
         6 = clusters handed to the quad fit (uint64[3] each: key, points, hash of the sorted point records), ordered by key
         9 = decimated gray before quad_sigma's filter (u8, B*sh*sw); the same as 0 while quad_sigma is off
         (7 and 8 named diagnostics that are gone; the numbers are not reused and stay ASL_EINVAL)
   bytes = capacity of dst in bytes; *n_items = number of elements written. */
typedef struct {
    double p[4][2]; /* decimated-image pixel coordinates, before the full-resolution rescale */
    uint64_t cluster;
    int32_t frame;
    int32_t reversed_border;
} asl_debug_quad;
int asl_debug_fetch(asl_detector *det, int what, void *dst, size_t bytes, size_t *n_items);

/* Diagnostic: re-run the quad fit of the last batch reps (>= 1) times on the device buffers it left behind.  It overwrites
   the last batch's quad records.  Clusters of more than 1024 points are not re-run: their fit sorts in place, so a second
   run would not see the same input.  out (n_out >= 7) = {repetitions, quads that differ from the first repetition, those
   by size class 0-4}; any difference is a race.  Fails if a batch is pending or the last batch had no clusters. */
int asl_debug_refit(asl_detector *det, int reps, int64_t *out, size_t n_out);
/* Diagnostic: the de-duplication stage (S8) alone on n records of the caller's, through the launches a batch uses.  dets[i]
   is one decoded tag of frame dets[i].frame in [0, n_frames) and keys[i] its cluster key, of which the low 48 bits count:
   within a frame the stage walks the records in ascending key order, whatever their order in memory (keys of one frame
   should differ).  cap_per_frame is the room of a frame's list, the capacity a batch grows on overflow; nothing grows
   here.  out (max_out >= n records) receives the survivors frame by frame, inside a frame by (id, hamming, corners), as a
   detect call returns them; n_per_frame (n_frames values) their counts; counters (n_counters >= 3) = {survivors, records
   that found their frame's list full, frames with more than 1024 records}.  A full list empties every frame and a frame
   above 1024 records is empty itself, as in a batch, which then grows and runs again or fails.  Synchronous; works in
   device buffers of its own, so the detector's workspace and the last batch's results and counters stay as they were.
   ASL_EINVAL, nothing written: a NULL pointer, n < 0, n_frames outside [1, 65535], cap_per_frame < 1, a frame index out
   of range, max_out < n, n_counters < 3, a batch pending. */
int asl_debug_dedup(asl_detector *det, const asl_detection *dets, const uint64_t *keys, int n, int n_frames, int cap_per_frame,
                    asl_detection *out, int max_out, int *n_per_frame, int64_t *counters, size_t n_counters);
/* Diagnostic: the dense linear algebra of the pose-graph back-end alone, on a matrix of the caller's: the blocked Cholesky
   (48-column blocks), the back substitution and the diag(A^-1) pass, launched as asl_gn_solve and asl_map_* launch them.
   A is n x n row-major, symmetric (the lower triangle is read), b has n values, n = 6 x tags with 1 <= tags <= 1000.
   L (n_L >= n * n): the factor, upper triangle zero;  y, x, var (n_vec >= n each): L^-1 b (the right-hand side rides through
   the factorisation as row n), the solution of A x = b, and diag(A^-1);  Linv (n_Linv >= ceil(n / 48) * 48 * 48): the
   inverses of the factor's diagonal blocks, 48 x 48 row-major each, a partial last block padded with the identity;
   *fail_flag: 1 if A is not positive definite (the call still returns ASL_OK: the other outputs are then meaningless).
   Synchronous, in device buffers of its own.  ASL_EINVAL, nothing written: a NULL pointer, n not such a size, an output
   too small, a batch pending. */
int asl_debug_gn_cholesky(asl_detector *det, const double *A, const double *b, int n, double *L, size_t n_L, double *y, double *x,
                          double *var, size_t n_vec, double *Linv, size_t n_Linv, int32_t *fail_flag);
/* Diagnostic: one damped step of asl_gn_solve's problem (its arguments and checks; cam_T and tag_T are only read), with the
   damping lambda (>= 0) given: the linearisation and its cost, the cameras eliminated, the reduced system factored, the
   step and the trial poses, through the launches a solve uses.  out has ASL_GN_STEP__N entries, one per item below; an
   entry {p, n} names room for n doubles at p, p NULL: not wanted.  Item (doubles needed):
     D (n_obs * 156) the 12 x 13 blocks [J^T J | J^T r] per observation;  COST_OBS (n_obs), COST (1) their costs and the sum;
     HINV (n_cams * 36), GC (n_cams * 6) the damped camera blocks inverted and the camera gradients;  TFJ (n_obs * 36)
     H_cc^-1 W_fj per observation;  S (n * n, n = 6 n_tags), RHS (n) the reduced system before it is factored;
     DG (n) the tag steps;  WN (n_cams * 12), GN (n_tags * 12) the trial poses camera<-world and world<-tag, R row-major then t.
   *fail_flag (may be NULL): 1 if the reduced system was not positive definite.  Synchronous, in a workspace of its own.
   ASL_EINVAL, nothing written: asl_gn_solve's refusals, out NULL, n_out != ASL_GN_STEP__N, lambda negative or not finite,
   an entry too small, a batch pending. */
typedef struct {
    double *p;
    size_t n;
} asl_debug_span;
enum { ASL_GN_STEP_D = 0, ASL_GN_STEP_COST_OBS, ASL_GN_STEP_COST, ASL_GN_STEP_HINV, ASL_GN_STEP_GC, ASL_GN_STEP_TFJ, ASL_GN_STEP_S,
       ASL_GN_STEP_RHS, ASL_GN_STEP_DG, ASL_GN_STEP_WN, ASL_GN_STEP_GN, ASL_GN_STEP__N };
int asl_debug_gn_step(asl_detector *det, int n_cams, int n_tags, int n_obs, const int32_t *obs_cam, const int32_t *obs_tag,
                      const double *obs_corners, const double *K, double tag_size, int fixed_tag, const double *cam_T,
                      const double *tag_T, double lambda, const asl_debug_span *out, int n_out, int32_t *fail_flag);
/* Diagnostic: the shared-reciprocal division of the line fits (asl_common.h) against the compiler's on 2^29 random operand
   pairs with exponents within +-exponent_limit (in [1, 900]).  out (n_out >= 2) = {pairs, mismatches}. */
int asl_debug_division_check(asl_detector *det, int exponent_limit, int64_t *out, size_t n_out);

/* Time of each stage of the last batch in milliseconds (HIP events on the detector's stream):
   names[i] / ms[i], i < *n. */
int asl_stage_times(asl_detector *det, const char **names, float *ms, int max_n, int *n);
/* Enable/disable per-stage event timing (adds a few events per batch; off by default). */
int asl_set_profiling(asl_detector *det, int enabled);

/* Diagnostic builds only (-DASL_PHASE_TIMING): summed shader-clock cycles per kernel phase into out (n_out >= 64
   counters); all zeros in the shipped library.  reset != 0 zeroes the counters afterwards. */
int asl_debug_phase_cycles(asl_detector *det, unsigned long long *out, size_t n_out, int reset);

#ifdef __cplusplus
}
#endif
#endif
