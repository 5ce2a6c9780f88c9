"""ctypes binding of libaprilslam.so (include/aprilslam.h).  No fallback: if the HIP library
is missing or no gfx950 device is usable, every call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ASL_LIB") or os.path.join(_HERE, "libaprilslam.so")  # ASL_LIB: diagnostic builds only


class AslError(RuntimeError):
    pass


PLANE_DTYPE = np.dtype([("Hi", "<f8", (9,)), ("bbox", "<i4", (4,)), ("tex", "<i4"), ("pad", "<i4")])  # asl_render_plane
assert PLANE_DTYPE.itemsize == 96
OBS_DTYPE = np.dtype([("id", "<i4"), ("flags", "<i4"), ("corners", "<f4", (8,)), ("T", "<f8", (12,))])  # asl_obs
assert OBS_DTYPE.itemsize == 136
DET_DTYPE = np.dtype([("id", "<i4"), ("hamming", "<i4"), ("margin", "<f4"), ("frame", "<i4"),
                      ("center", "<f8", (2,)), ("corners", "<f8", (4, 2))])
POSE_DTYPE = np.dtype([("rvec", "<f8", (3,)), ("tvec", "<f8", (3,)), ("T", "<f8", (4, 4)), ("ok", "<i4"), ("reserved", "<i4")])
MAP_TAG_DTYPE = np.dtype([("T", "<f8", (12,)), ("valid", "<i4"), ("size", "<f4")])  # asl_map_tag; size 0: the call's tag_size
CAM_POSE_DTYPE = np.dtype([("T", "<f8", (4, 4)), ("rms_px", "<f8"), ("rms_seed_px", "<f8"), ("n_tags", "<i4"), ("n_rejected", "<i4"),
                           ("status", "<i4"), ("seed_slot", "<i4")])  # asl_cam_pose
CALIB_RESULT_DTYPE = np.dtype([("K", "<f8", (3, 3)), ("dist", "<f8", (5,)), ("std", "<f8", (9,)), ("rms_px", "<f8"),
                               ("rms_init_px", "<f8"), ("n_frames_used", "<i4"), ("n_corners", "<i4"), ("iterations", "<i4"),
                               ("status", "<i4")])  # asl_calib_result
MAP_RESULT_DTYPE = np.dtype([("cost_seed", "<f8"), ("cost", "<f8"), ("rms_px", "<f8"), ("rms_seed_px", "<f8"),
                             ("n_frames_used", "<i4"), ("n_tags", "<i4"), ("n_obs", "<i4"), ("n_obs_dropped", "<i4"),
                             ("iterations", "<i4"), ("world_id", "<i4"), ("status", "<i4"), ("n_soft", "<i4")])  # asl_map_result
SMOOTH_RESULT_DTYPE = np.dtype([("cost_seed", "<f8"), ("cost", "<f8"), ("rms_px", "<f8"), ("rms_seed_px", "<f8"),
                                ("n_frames_data", "<i4"), ("n_filled", "<i4"), ("n_flipped", "<i4"), ("iterations", "<i4"),
                                ("status", "<i4"), ("n_soft", "<i4"), ("reserved", "<i4", (2,))])  # asl_smooth_result
POSE_COV_DTYPE = np.dtype([("cov", "<f8", (6, 6)), ("sigma_px", "<f8"), ("dof", "<i4"), ("status", "<i4")])  # asl_pose_cov
QUAD_DTYPE = np.dtype([("p", "<f8", (4, 2)), ("cluster", "<u8"), ("frame", "<i4"), ("reversed_border", "<i4")])  # asl_debug_quad
assert DET_DTYPE.itemsize == 96 and POSE_DTYPE.itemsize == 184 and QUAD_DTYPE.itemsize == 80  # asl_detection, asl_pose, asl_debug_quad
assert MAP_TAG_DTYPE.itemsize == 104
assert CAM_POSE_DTYPE.itemsize == 160
assert CALIB_RESULT_DTYPE.itemsize == 216
assert MAP_RESULT_DTYPE.itemsize == 64
assert SMOOTH_RESULT_DTYPE.itemsize == 64
assert POSE_COV_DTYPE.itemsize == 304
RIG_CAMERA_DTYPE = np.dtype([("K", "<f8", (3, 3)), ("dist", "<f8", (5,)), ("E", "<f8", (3, 4)), ("n_dist", "<i4"), ("reserved", "<i4")])  # asl_rig_camera
assert RIG_CAMERA_DTYPE.itemsize == 216
BUNDLE_REL_DTYPE = np.dtype([("T", "<f8", (4, 4)), ("cov", "<f8", (6, 6)), ("status", "<i4"), ("reserved", "<i4")])  # asl_bundle_rel; T = ref<-bundle
assert BUNDLE_REL_DTYPE.itemsize == 424
RIG_CALIB_RESULT_DTYPE = np.dtype([("rms_px", "<f8"), ("rms_init_px", "<f8"), ("sigma_px", "<f8"), ("n_frames_used", "<i4"), ("n_corners", "<i4"),
                                   ("iterations", "<i4"), ("status", "<i4"), ("n_solved", "<i4"), ("reserved", "<i4"),
                                   ("cam_status", "<i4", (16,)), ("cam_frames", "<i4", (16,))])  # asl_rig_calib_result
assert RIG_CALIB_RESULT_DTYPE.itemsize == 176
TAG_FIT_DTYPE = np.dtype([("rms_px", "<f8"), ("rms_seed_px", "<f8"), ("n_views", "<i4"), ("n_rejected", "<i4"), ("status", "<i4"),
                          ("seed_frame", "<i4"), ("seed_mirrored", "<i4"), ("reserved", "<i4")])  # asl_tag_fit
assert TAG_FIT_DTYPE.itemsize == 40

RECTIFY_VIEW_DTYPE = np.dtype([("K", "<f8", (3, 3)), ("R", "<f8", (3, 3))])  # asl_rectify_view; R = source camera <- view
assert RECTIFY_VIEW_DTYPE.itemsize == 144
LENS_BROWN, LENS_FISHEYE, MAX_VIEWS = 0, 1, 16   # ASL_LENS_BROWN, ASL_LENS_FISHEYE, ASL_MAX_VIEWS
LENS_MODELS = {"brown": LENS_BROWN, "fisheye": LENS_FISHEYE}
EXPORTS = [
    "asl_detector_create", "asl_family_check", "asl_detector_create_family", "asl_families_check", "asl_detector_create_families", "asl_detector_family_of", "asl_detector_destroy", "asl_detector_set_id_limit", "asl_detector_set_pnp_both_minima", "asl_detector_set_quad_sigma", "asl_blur_taps", "asl_last_error", "asl_version", "asl_detect_gray_u8",
    "asl_detect_bgr_u8", "asl_detect_batch_u8", "asl_detect_batch_pose_u8", "asl_detect_batch_device", "asl_submit_batch_device", "asl_collect_batch", "asl_collect_batch_view", "asl_solve_pnp_batch", "asl_gn_solve", "asl_pack_observations_device", "asl_graph_frames_device", "asl_graph_picks_device", "asl_render_frames_device",
    "asl_rectify_frames_device", "asl_rectify_u8", "asl_rectify_views_device", "asl_rectify_views_u8",
    "asl_localize_frames_device", "asl_localize_batch", "asl_localize_cov_frames_device", "asl_localize_cov_batch",
    "asl_localize_mapcov_frames_device", "asl_localize_mapcov_batch", "asl_localize_rig_mapcov_frames_device", "asl_localize_rig_mapcov_batch",
    "asl_pose_cov_device", "asl_solve_pnp_cov_batch", "asl_calibrate_frames_device", "asl_calibrate_batch",
    "asl_calibrate_lens_frames_device", "asl_calibrate_lens_batch",
    "asl_localize_rig_frames_device", "asl_localize_rig_cov_frames_device", "asl_localize_rig_batch", "asl_localize_rig_cov_batch",
    "asl_localize_bundles_frames_device", "asl_localize_bundles_batch", "asl_localize_bundles_rig_frames_device", "asl_localize_bundles_rig_batch",
    "asl_bundle_relative_device", "asl_bundle_relative_batch",
    "asl_calibrate_rig_frames_device", "asl_calibrate_rig_batch",
    "asl_map_frames_device", "asl_map_batch", "asl_map_robust_frames_device", "asl_map_robust_batch", "asl_map_rig_frames_device", "asl_map_rig_batch", "asl_map_sized_frames_device", "asl_map_sized_batch",
    "asl_map_rig_sized_frames_device", "asl_map_rig_sized_batch",
    "asl_mapcov_frames_device", "asl_mapcov_batch", "asl_mapcov_rig_frames_device", "asl_mapcov_rig_batch", "asl_smooth_frames_device", "asl_smooth_batch", "asl_smooth_cov_frames_device", "asl_smooth_cov_batch",
    "asl_smooth_sequences_device", "asl_smooth_sequences_batch", "asl_smooth_robust_sequences_device", "asl_smooth_robust_sequences_batch",
    "asl_smooth_timed_sequences_device", "asl_smooth_timed_sequences_batch",
    "asl_smooth_rig_sequences_device", "asl_smooth_rig_sequences_batch",
    "asl_locate_tags_frames_device", "asl_locate_tags_batch", "asl_locate_tags_rig_frames_device", "asl_locate_tags_rig_batch",
    "asl_debug_fetch", "asl_debug_refit", "asl_debug_dedup", "asl_debug_gn_cholesky", "asl_debug_gn_step", "asl_debug_division_check", "asl_stage_times", "asl_set_profiling", "asl_debug_phase_cycles",
]



MAX_FAMILIES = 4  # ASL_MAX_FAMILIES
BUILTIN_FAMILY = "tagStandard41h12"  # asl_detector_create's one name; every other family goes in as a table


class AslFamily(C.Structure):    # asl_family
    _fields_ = [("nbits", C.c_int32), ("width_at_border", C.c_int32), ("total_width", C.c_int32), ("reversed_border", C.c_int32),
                ("ncodes", C.c_int32), ("reserved", C.c_int32), ("bit_x", C.POINTER(C.c_int32)), ("bit_y", C.POINTER(C.c_int32)),
                ("codes", C.POINTER(C.c_uint64))]


class FamilyTable:
    """An asl_family over a TagFamily (families.py), with the arrays it points into kept alive."""

    def __init__(self, fam):
        self.bit_x = np.ascontiguousarray(fam.bit_x, dtype=np.int32)
        self.bit_y = np.ascontiguousarray(fam.bit_y, dtype=np.int32)
        self.codes = np.ascontiguousarray(fam.codes, dtype=np.uint64)
        self.c = AslFamily(int(fam.nbits), int(fam.width_at_border), int(fam.total_width), int(bool(fam.reversed_border)),
                           int(self.codes.shape[0]), 0, self.bit_x.ctypes.data_as(C.POINTER(C.c_int32)),
                           self.bit_y.ctypes.data_as(C.POINTER(C.c_int32)), self.codes.ctypes.data_as(C.POINTER(C.c_uint64)))


def family_check(fam):
    """asl_family_check on a TagFamily: raises AslError naming the field the detector cannot take.  No GPU needed."""
    check(load().asl_family_check(C.byref(FamilyTable(fam).c)))


def _tag_family(family):
    """A TagFamily of a TagFamily or a registered (or the built-in) name."""
    if not isinstance(family, str):
        return family
    from . import families
    if family != BUILTIN_FAMILY and not families.is_registered(family):
        raise AslError("unknown tag family '%s'" % family)
    return families.get_family(family)


class FamilySet:
    """What asl_families_check / asl_detector_create_families take: an asl_family array over TagFamily objects or names,
    with their id bases.  id_base None: the cumulative bases 0, n0, n0 + n1, ..."""

    def __init__(self, fams, id_base=None):
        self.families = tuple(_tag_family(f) for f in fams)
        self.tables = [FamilyTable(f) for f in self.families]
        if id_base is None:
            id_base = np.cumsum([0] + [len(t.codes) for t in self.tables[:-1]]) if self.tables else []
        if len(id_base) != len(self.tables):
            raise ValueError("one id_base per family")
        self.id_base = np.ascontiguousarray(id_base, dtype=np.int32)
        self.c = (AslFamily * max(len(self.tables), 1))(*[t.c for t in self.tables])
        self.n = len(self.tables)

    @property
    def id_base_p(self):
        return self.id_base.ctypes.data_as(C.POINTER(C.c_int32))


def families_check(fams, id_base=None):
    """asl_families_check on a list of TagFamily objects / names: raises AslError naming the family's index and the field.
    No GPU needed."""
    fs = FamilySet(fams, id_base)
    check(load().asl_families_check(fs.c, fs.id_base_p, fs.n))


class DebugSpan(C.Structure):    # asl_debug_span: room for n doubles at p; p NULL: not wanted
    _fields_ = [("p", C.POINTER(C.c_double)), ("n", C.c_size_t)]


# asl_debug_gn_step's items in the header's order (ASL_GN_STEP_*), with the shape of each for (P cameras, L tags, M observations)
GN_STEP_ITEMS = ("D", "cost_obs", "cost", "Hinv", "gc", "Tfj", "S", "rhs", "dG", "Wn", "Gn")


def gn_step_shapes(P, L, M):
    return dict(D=(M, 12, 13), cost_obs=(M,), cost=(1,), Hinv=(P, 6, 6), gc=(P, 6), Tfj=(M, 6, 6), S=(6 * L, 6 * L), rhs=(6 * L,),
                dG=(L, 6), Wn=(P, 12), Gn=(L, 12))


_lib = None


def load():
    """Load libaprilslam.so and declare the prototypes.  Raises AslError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AslError("libaprilslam.so is not built (%s missing): run `python -c 'import __graft_entry__ as g; g.build()'`"
                       % LIB_PATH)
    # ONE HIP runtime per process: PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1, and a
    # second runtime initialised in the same process cannot see the GPU.  Importing torch first makes
    # libaprilslam.so's NEEDED "libamdhip64.so.7" resolve to the copy torch already loaded (same SONAME).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, dp, u8p = C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    L.asl_last_error.restype = C.c_char_p
    L.asl_version.restype = C.c_char_p
    L.asl_detector_create.argtypes = [C.c_char_p, i32, i32, C.c_float, C.c_float, i32, i32, C.POINTER(vp)]
    L.asl_family_check.argtypes = [C.POINTER(AslFamily)]
    L.asl_detector_create_family.argtypes = [C.POINTER(AslFamily), i32, i32, C.c_float, C.c_float, i32, i32, C.POINTER(vp)]
    L.asl_families_check.argtypes = [C.POINTER(AslFamily), C.POINTER(C.c_int32), i32]
    L.asl_detector_create_families.argtypes = [C.POINTER(AslFamily), C.POINTER(C.c_int32), i32, i32, i32, C.c_float, C.c_float, i32, i32, C.POINTER(vp)]
    L.asl_detector_family_of.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.asl_detector_destroy.argtypes = [vp]
    L.asl_detector_destroy.restype = None
    L.asl_detector_set_id_limit.argtypes = [vp, i32]
    L.asl_detector_set_pnp_both_minima.argtypes = [vp, i32]
    L.asl_detector_set_quad_sigma.argtypes = [vp, C.c_float]
    L.asl_blur_taps.argtypes = [C.c_float, u8p, i32, C.POINTER(i32)]
    L.asl_detect_gray_u8.argtypes = [vp, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
    L.asl_detect_bgr_u8.argtypes = [vp, vp, i32, i32, i32, vp, i32, C.POINTER(i32)]
    L.asl_detect_batch_u8.argtypes = [vp, C.POINTER(vp), i32, i32, i32, i32, i32, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.asl_detect_batch_pose_u8.argtypes = [vp, C.POINTER(vp), i32, i32, i32, i32, i32, dp, dp, i32, C.c_double, vp, vp, i32,
                                           C.POINTER(i32), C.POINTER(i32)]
    L.asl_detect_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_size_t, vp, dp, dp, i32, C.c_double,
                                          vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.asl_submit_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_size_t, vp, dp, dp, i32, C.c_double]
    L.asl_collect_batch.argtypes = [vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.asl_collect_batch_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
    L.asl_solve_pnp_batch.argtypes = [vp, C.POINTER(C.c_float), dp, dp, i32, C.c_double, dp, dp, dp, u8p, i32]
    L.asl_gn_solve.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp, C.c_double, i32,
                               dp, dp, i32, dp]
    L.asl_render_frames_device.argtypes = [vp, vp, i32, i32, i32, i32, C.c_size_t, vp, i32, vp, i32, i32, C.c_double, dp, dp, i32, vp]
    L.asl_rectify_frames_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_size_t, vp, i32, i32, i32, C.c_size_t, dp, dp, i32, dp, i32, vp]
    L.asl_rectify_u8.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, dp, dp, i32, dp, i32]
    L.asl_rectify_views_device.argtypes = [vp, vp, i32, i32, i32, i32, i32, C.c_size_t, vp, i32, i32, i32, C.c_size_t, dp, dp, i32, i32, vp, i32,
                                           C.c_double, i32, vp]
    L.asl_rectify_views_u8.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, C.c_size_t, dp, dp, i32, i32, vp, i32, C.c_double, i32]
    L.asl_pack_observations_device.argtypes = [vp, vp, i32, vp]
    L.asl_graph_frames_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]
    L.asl_graph_picks_device.argtypes = [vp, vp, i32, i32, i32, vp, C.c_uint32, C.c_uint32, vp, i32, vp, vp]
    # the solver entries (csrc/solve_host.inc), from the pieces their argument lists share
    dbl, obs_block, tag_map = C.c_double, [vp, i32, i32], [vp, i32]    # obs, n_frames, max_tags; map, n_ids
    camera, sigmas = [dp, dp, i32, dbl], [dbl, dbl, dbl]          # K, dist, n_dist, tag_size; sigma_px, sigma_rot, sigma_trans
    loc = [vp] + obs_block + tag_map + camera + [dbl]             # detector, ..., max_tag_rms_px
    L.asl_localize_frames_device.argtypes = loc + [vp, vp]
    L.asl_localize_batch.argtypes = loc + [vp]
    L.asl_localize_cov_frames_device.argtypes = loc + [dbl, vp, vp, vp]
    L.asl_localize_cov_batch.argtypes = loc + [dbl, vp, vp]
    map_cov_in = [vp, i32, vp]                                    # map_cov, ld, cov_slot: after the _cov forms' cov
    L.asl_localize_mapcov_frames_device.argtypes = loc + [dbl, vp, vp] + map_cov_in + [vp]
    L.asl_localize_mapcov_batch.argtypes = loc + [dbl, vp, vp] + map_cov_in
    rig = [vp, vp, i32, i32, i32] + tag_map + [vp, dbl, dbl]      # detector, obs, n_cams, n_frames, max_tags, ..., rig, tag_size, max_tag_rms_px
    L.asl_localize_rig_frames_device.argtypes = rig + [vp, vp]
    L.asl_localize_rig_batch.argtypes = rig + [vp]
    L.asl_localize_rig_cov_frames_device.argtypes = rig + [dbl, vp, vp, vp]
    L.asl_localize_rig_cov_batch.argtypes = rig + [dbl, vp, vp]
    L.asl_localize_rig_mapcov_frames_device.argtypes = rig + [dbl, vp, vp] + map_cov_in + [vp]
    L.asl_localize_rig_mapcov_batch.argtypes = rig + [dbl, vp, vp] + map_cov_in
    bundles = loc[:5] + [i32] + loc[5:] + [dbl, vp, vp]             # ..., maps, n_bundles, n_ids, ..., max_tag_rms_px, sigma_px, out, cov
    L.asl_localize_bundles_frames_device.argtypes = bundles + [vp]
    L.asl_localize_bundles_batch.argtypes = bundles
    bundles_rig = rig[:6] + [i32] + rig[6:] + [dbl, vp, vp]
    L.asl_localize_bundles_rig_frames_device.argtypes = bundles_rig + [vp]
    L.asl_localize_bundles_rig_batch.argtypes = bundles_rig
    L.asl_bundle_relative_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]    # detector, poses, cov, n_frames, n_bundles, ref, rel, stream
    L.asl_bundle_relative_batch.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.asl_pose_cov_device.argtypes = [vp, vp, i32] + camera + [dbl, vp, vp]
    L.asl_solve_pnp_cov_batch.argtypes = [vp, C.POINTER(C.c_float), dp] + camera + [dbl, vp, i32]
    calib = [vp] + obs_block + tag_map + [dbl, i32, i32, dp, i32, i32, i32, vp, vp]    # ..., tag_size, width, height, K_init, n_dist, flags, max_iters, the two results
    L.asl_calibrate_frames_device.argtypes = calib + [vp]
    L.asl_calibrate_batch.argtypes = calib
    calib_lens = calib[:10] + [i32] + calib[10:]                  # ..., K_init, lens_model, n_dist, ...
    L.asl_calibrate_lens_frames_device.argtypes = calib_lens + [vp]
    L.asl_calibrate_lens_batch.argtypes = calib_lens
    calib_rig = rig[:9] + [i32, dbl, vp, vp, vp, vp]              # ..., rig, tag_size, max_iters, sigma_px, rig_out, result, cov, poses
    L.asl_calibrate_rig_frames_device.argtypes = calib_rig + [vp]
    L.asl_calibrate_rig_batch.argtypes = calib_rig
    mapping = [vp] + obs_block + [i32] + camera + [i32, i32, vp, vp, vp, vp]    # ..., n_ids, camera, world_id, max_iters, the four results
    L.asl_map_frames_device.argtypes = mapping + [vp]
    L.asl_map_batch.argtypes = mapping
    mapping_robust = mapping[:10] + [dbl] + mapping[10:] + [vp]    # ..., world_id, huber_px, max_iters, the four results, slot_weight
    L.asl_map_robust_frames_device.argtypes = mapping_robust + [vp]
    L.asl_map_robust_batch.argtypes = mapping_robust
    mapping_rig = [vp, vp, i32, i32, i32, i32, vp, dbl] + mapping_robust[9:]    # detector, obs, n_cams, n_frames, max_tags, n_ids, rig, tag_size, world_id, ...
    L.asl_map_rig_frames_device.argtypes = mapping_rig + [vp]
    L.asl_map_rig_batch.argtypes = mapping_rig
    fp = C.POINTER(C.c_float)                                     # tag_sizes, after tag_size: a host array in the device forms too
    L.asl_map_sized_frames_device.argtypes = mapping_robust[:9] + [fp] + mapping_robust[9:] + [vp]
    L.asl_map_sized_batch.argtypes = mapping_robust[:9] + [fp] + mapping_robust[9:]
    L.asl_map_rig_sized_frames_device.argtypes = mapping_rig[:8] + [fp] + mapping_rig[8:] + [vp]
    L.asl_map_rig_sized_batch.argtypes = mapping_rig[:8] + [fp] + mapping_rig[8:]
    map_cov = [vp, vp, i32]                                       # cov_slot, map_cov, cap_tags: after the sized forms' slot_weight
    L.asl_mapcov_frames_device.argtypes = L.asl_map_sized_batch.argtypes + map_cov + [vp]
    L.asl_mapcov_batch.argtypes = L.asl_map_sized_batch.argtypes + map_cov
    L.asl_mapcov_rig_frames_device.argtypes = L.asl_map_rig_sized_batch.argtypes + map_cov + [vp]
    L.asl_mapcov_rig_batch.argtypes = L.asl_map_rig_sized_batch.argtypes + map_cov
    smooth, seqs = [vp] + obs_block + tag_map + camera + [vp], [C.POINTER(C.c_int32), i32]    # ..., seed; seq_start, n_seq
    solve = sigmas + [i32, vp, vp]                                # ..., max_iters, out, result
    L.asl_smooth_frames_device.argtypes = smooth + solve + [vp]
    L.asl_smooth_batch.argtypes = smooth + solve
    L.asl_smooth_cov_frames_device.argtypes = smooth + solve + [vp, vp]
    L.asl_smooth_cov_batch.argtypes = smooth + solve + [vp]
    L.asl_smooth_sequences_device.argtypes = smooth + seqs + solve + [vp, vp]
    L.asl_smooth_sequences_batch.argtypes = smooth + seqs + solve + [vp]
    robust = sigmas + [dbl] + solve[3:]                           # ..., sigma_trans, huber_px, max_iters, out, results
    L.asl_smooth_robust_sequences_device.argtypes = smooth + seqs + robust + [vp, vp]
    L.asl_smooth_robust_sequences_batch.argtypes = smooth + seqs + robust + [vp]
    L.asl_smooth_timed_sequences_device.argtypes = smooth + [vp] + seqs + robust + [vp, vp]    # ..., seed, times, seq_start, ...
    L.asl_smooth_timed_sequences_batch.argtypes = smooth + [dp] + seqs + robust + [vp]
    smooth_rig = rig[:8] + [dbl, vp]                              # detector, obs, n_cams, n_frames, max_tags, map, n_ids, rig, tag_size, seed
    L.asl_smooth_rig_sequences_device.argtypes = smooth_rig + [vp] + seqs + robust + [vp, vp]    # ..., seed, frame_times, seq_start, ...
    L.asl_smooth_rig_sequences_batch.argtypes = smooth_rig + [dp] + seqs + robust + [vp]
    locate = [vp] + obs_block + [vp] + tag_map + camera + [dbl, i32, dbl, vp, vp]    # ..., poses, map, n_ids, camera, gate, min_views, sigma_px, fit, cov
    L.asl_locate_tags_frames_device.argtypes = locate + [vp]
    L.asl_locate_tags_batch.argtypes = locate
    locate_rig = [vp, vp, i32, i32, i32] + locate[4:7] + [vp, dbl] + locate[11:]    # detector, obs, n_cams, n_frames, max_tags, poses, map, n_ids, rig, tag_size, ...
    L.asl_locate_tags_rig_frames_device.argtypes = locate_rig + [vp]
    L.asl_locate_tags_rig_batch.argtypes = locate_rig
    L.asl_debug_fetch.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.asl_debug_refit.argtypes = [vp, i32, vp, C.c_size_t]
    L.asl_debug_dedup.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, C.c_size_t]
    L.asl_debug_gn_cholesky.argtypes = [vp, dp, dp, i32, dp, C.c_size_t, dp, dp, dp, C.c_size_t, dp, C.c_size_t, C.POINTER(C.c_int32)]
    L.asl_debug_gn_step.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp, C.c_double, i32, dp, dp,
                                    C.c_double, C.POINTER(DebugSpan), i32, C.POINTER(C.c_int32)]
    L.asl_debug_division_check.argtypes = [vp, i32, vp, C.c_size_t]
    L.asl_stage_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32, C.POINTER(i32)]
    L.asl_set_profiling.argtypes = [vp, i32]
    L.asl_debug_phase_cycles.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, i32]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise AslError("libaprilslam error %d: %s" % (rc, load().asl_last_error().decode("utf-8", "replace")))


_DP = C.POINTER(C.c_double)


def blur_taps(quad_sigma):
    """asl_blur_taps: the uint8 taps k_quad_blur uses for this quad_sigma (empty: off).  A host function: no GPU needed."""
    taps = np.zeros(15, dtype=np.uint8)
    ksz = C.c_int()
    check(load().asl_blur_taps(float(quad_sigma), taps.ctypes.data_as(C.POINTER(C.c_uint8)), len(taps), C.byref(ksz)))
    return taps[:ksz.value].copy()


def _ptr(addr):
    """a device address"""
    return C.c_void_p(int(addr))


def _data(a):
    """the address of a host array's data, or NULL for an empty one"""
    return a.ctypes.data if a.size else None


def _opt_ptr(addr):
    """a device address, or NULL for 0 / None"""
    return C.c_void_p(int(addr)) if addr else None


def _camera(K, dist, square=False):
    """K and dist as the C ABI takes them: (arrays to keep alive, K pointer, dist pointer or None, n_dist).  dist: None or
    0, 4 or 5 coefficients; square: K must be 3x3."""
    Kc = np.ascontiguousarray(K, dtype=np.float64)
    if square and Kc.shape != (3, 3):
        raise ValueError("K must be 3x3")
    dc = np.ascontiguousarray(np.zeros(0) if dist is None else dist, dtype=np.float64).ravel()
    if len(dc) not in (0, 4, 5):
        raise ValueError("dist must have 0, 4 or 5 coefficients")
    return (Kc, dc), Kc.ctypes.data_as(_DP), (dc.ctypes.data_as(_DP) if len(dc) else None), len(dc)


def _lens(K, dist, model):
    """_camera for a lens of either model: (arrays to keep alive, K pointer, dist pointer or None, n_dist, lens_model).
    model: "brown" (0, 4 or 5 coefficients k1 k2 p1 p2 [k3]) or "fisheye" (0 or 4: k1 k2 k3 k4), or the ABI's number."""
    m = LENS_MODELS.get(model, model)
    if m not in (LENS_BROWN, LENS_FISHEYE):
        raise ValueError("model must be 'brown' or 'fisheye'")
    keep, Kp, dpp, nd = _camera(K, dist, square=True)
    if m == LENS_FISHEYE and nd not in (0, 4):
        raise ValueError("a fisheye lens has 0 or 4 coefficients (k1, k2, k3, k4)")
    return keep, Kp, dpp, nd, m


def rectify_view_records(views):
    """[(K_new, R)] or RECTIFY_VIEW_DTYPE records -> contiguous (n_views,) RECTIFY_VIEW_DTYPE"""
    if isinstance(views, np.ndarray) and views.dtype == RECTIFY_VIEW_DTYPE:
        return np.ascontiguousarray(views).ravel()
    rec = np.zeros(len(views), dtype=RECTIFY_VIEW_DTYPE)
    for k, (K_new, R) in enumerate(views):
        rec["K"][k] = np.asarray(K_new, dtype=np.float64).reshape(3, 3)
        rec["R"][k] = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    return rec


def _obs_records(obs):
    """host asl_obs records as one contiguous (n_frames, max_tags) block; one frame's row may be 1-D"""
    o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
    if o.ndim == 1:
        o = o[None]
    if o.ndim != 2:
        raise ValueError("obs must be (n_frames, max_tags) asl_obs records")
    return o


def _map_cov_args(map_cov, n_ids):
    """(cov_slot (n_ids,) int32, matrix C-contiguous float64, ld) of a mapping.MapCovariance or a (cov_slot, matrix) pair"""
    if hasattr(map_cov, "as_args"):
        return map_cov.as_args(n_ids)
    slot, mat = map_cov
    slot = np.ascontiguousarray(slot, dtype=np.int32).ravel()
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    if len(slot) != n_ids:
        raise ValueError("cov_slot has %d entries, the map %d" % (len(slot), n_ids))
    if mat.ndim != 2 or mat.shape[0] != mat.shape[1] or mat.shape[0] % 6:
        raise ValueError("the map covariance must be a square matrix of 6 x 6 blocks")
    if mat.shape[0] == 0:
        mat = np.zeros((6, 6))
    return slot, mat, mat.shape[1]


def _map_records(tag_map):
    """(n_ids,) MAP_TAG_DTYPE records of a record array or a localize.TagMap"""
    if hasattr(tag_map, "as_records"):
        tag_map = tag_map.as_records()
    return np.ascontiguousarray(tag_map, dtype=MAP_TAG_DTYPE).ravel()


def _size_table(tag_sizes, n_ids):
    """(n_ids,) float32 table of the sized map calls from a {id: size} dict (ids >= n_ids are ignored, ids not named are 0:
    the call's tag_size) or an array of n_ids sizes; the library refuses negative and non-finite entries"""
    n = max(int(n_ids), 1)
    if isinstance(tag_sizes, dict):
        table = np.zeros(n, dtype=np.float32)
        for i, size in tag_sizes.items():
            if int(i) < 0:
                raise ValueError("tag_sizes: tag id %d is negative" % int(i))
            if int(i) < n:
                table[int(i)] = size
        return table
    table = np.ascontiguousarray(tag_sizes, dtype=np.float32).ravel()
    if len(table) != n:
        raise ValueError("tag_sizes must be a {id: size} dict or an array of n_ids = %d sizes (got %d)" % (n, len(table)))
    return table


def _bundle_tables(bundles, n_ids=None):
    """(n_bundles, n_ids) MAP_TAG_DTYPE, C-contiguous, of a bundles.BundleSet or of such a block (table b: bundle_b<-tag)"""
    if hasattr(bundles, "table"):
        return bundles.table(n_ids)
    t = np.ascontiguousarray(bundles, dtype=MAP_TAG_DTYPE)
    if t.ndim != 2:
        raise ValueError("bundles must be a BundleSet or (n_bundles, n_ids) asl_map_tag records")
    return t


def _rig_records(rig):
    """(n_cams,) RIG_CAMERA_DTYPE records of a record array or a rig.Rig"""
    if hasattr(rig, "as_records"):
        rig = rig.as_records()
    return np.ascontiguousarray(rig, dtype=RIG_CAMERA_DTYPE).ravel()


class Detector:
    """Owns one asl_detector (one GPU workspace).  Not re-entrant."""

    def __init__(self, family="tagStandard41h12", threads=1, maxhamming=1, decimate=2.0, blur=0.0, refine_edges=True,
                 device=0, id_limit=None, id_base=None):
        """family: the built-in name, the name of a family registered with families.register / families.load, or a
        TagFamily; or a list / tuple of those, for one detector that decodes several families in one pass and reports a
        tag with local id k of family i as id_base[i] + k (id_base None: the cumulative bases 0, n0, n0 + n1, ...); the
        built-in name in a list stands for its whole table.
        id_limit (one family only): None = the built-in family's ids the reference pins (0..4), every id of any other
        family; 0 = the whole table; n = ids 0..n-1."""
        L = load()
        self._L = L
        self._h = C.c_void_p()
        self._outbuf = self._posebuf = None  # detection / pose results kept across calls (_result_buffers)
        rest = (int(threads), int(maxhamming), float(decimate), float(blur), 1 if refine_edges else 0, int(device), C.byref(self._h))
        table = None
        if isinstance(family, (list, tuple)):
            fs = FamilySet(family, id_base)
            check(L.asl_detector_create_families(fs.c, fs.id_base_p, fs.n, *rest))  # the detector keeps its own copy of the tables
            self.families, self.id_base = fs.families, tuple(int(b) for b in fs.id_base)
            self.device = int(device)
            if id_limit is not None:
                check(L.asl_detector_set_id_limit(self._h, int(id_limit)))
            return
        if id_base is not None:
            raise ValueError("id_base goes with a list of families")
        if not isinstance(family, str):
            table = FamilyTable(family)
        elif family != BUILTIN_FAMILY:
            from . import families
            if families.is_registered(family):
                table = FamilyTable(families.get_family(family))
        if table is None:
            check(L.asl_detector_create(family.encode(), *rest))  # refuses an unknown name
        else:
            check(L.asl_detector_create_family(C.byref(table.c), *rest))  # the detector keeps its own copy of the table
        self.families, self.id_base = (_tag_family(family),), (0,)
        self.device = int(device)
        if id_limit is not None:
            check(L.asl_detector_set_id_limit(self._h, int(id_limit)))

    def family_of(self, id):
        """asl_detector_family_of: (index into the detector's families, the id inside that family) of a reported id."""
        fi, k = C.c_int(), C.c_int()
        check(self._L.asl_detector_family_of(self._h, int(id), C.byref(fi), C.byref(k)))
        return fi.value, k.value

    def set_pnp_both_minima(self, enabled):
        """asl_detector_set_pnp_both_minima: off = the reference's (cv2's) single minimum, on = the better of the two planar poses"""
        check(self._L.asl_detector_set_pnp_both_minima(self._h, 1 if enabled else 0))

    def set_quad_sigma(self, quad_sigma):
        """asl_detector_set_quad_sigma: Gaussian blur (> 0) or sharpening (< 0) of the decimated image from the next batch on;
        0 = off.  |quad_sigma| < 4."""
        check(self._L.asl_detector_set_quad_sigma(self._h, float(quad_sigma)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.asl_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host images ------------------------------------------------------------------
    def detect_host(self, images, max_per_frame=256, channels=None, K=None, dist=None, tag_size=0.0):
        """images: (H,W) / (H,W,3) uint8 array, or (B,H,W[,3]); pass channels=1 for a gray batch whose W is 3.
        Returns (dets, n_per_frame); with a camera matrix K the per-tag PnP runs in the same submission
        (asl_detect_batch_pose_u8) and the result is (dets, poses, n_per_frame)."""
        a = np.ascontiguousarray(images, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        elif a.ndim == 3 and a.shape[2] == 3 and channels != 1:
            a = a[None]
        if a.ndim == 3:
            ch = 1
            B, H, W = a.shape
        elif a.ndim == 4 and a.shape[3] == 3:
            ch = 3
            B, H, W = a.shape[:3]
        else:
            raise ValueError("expected (H,W), (H,W,3), (B,H,W) or (B,H,W,3) uint8")
        stride = W * ch
        ptrs = (C.c_void_p * B)(*[a[i].ctypes.data for i in range(B)])
        cap = B * max_per_frame
        out = np.empty(cap, dtype=DET_DTYPE)
        npf = (C.c_int * B)()
        n = C.c_int()
        if K is not None:
            keep, Kp, dpp, nd = _camera(K, dist)
            poses = np.empty(cap, dtype=POSE_DTYPE)
            check(self._L.asl_detect_batch_pose_u8(self._h, ptrs, B, ch, W, H, stride, Kp, dpp, nd, float(tag_size),
                                                   out.ctypes.data, poses.ctypes.data, cap, npf, C.byref(n)))
            if n.value > cap:
                return self.detect_host(images, (n.value + B - 1) // B + 1, channels, K, dist, tag_size)
            return out[:n.value], poses[:n.value], np.array(list(npf), dtype=np.int64)
        check(self._L.asl_detect_batch_u8(self._h, ptrs, B, ch, W, H, stride, out.ctypes.data, cap, npf, C.byref(n)))
        if n.value > cap:
            return self.detect_host(images, max_per_frame=(n.value + B - 1) // B + 1, channels=channels)
        return out[:n.value], np.array(list(npf), dtype=np.int64)

    # -- frames resident in HBM ---------------------------------------------------------
    def detect_device(self, data_ptr, n_frames, channels, width, height, stride=None, frame_pitch=None, stream=0,
                      K=None, dist=None, tag_size=0.0, max_per_frame=64, want_poses=None, reuse_buffers=False):
        stride = stride or width * channels
        frame_pitch = frame_pitch or stride * height
        cap = n_frames * max_per_frame
        want_poses = (K is not None) if want_poses is None else want_poses
        if reuse_buffers:  # the returned arrays are views into the kept buffers, valid until the next call on this detector
            out, poses = self._result_buffers(cap, want_poses)
        else:
            out, poses = np.empty(cap, dtype=DET_DTYPE), (np.empty(cap, dtype=POSE_DTYPE) if want_poses else None)
        npf = (C.c_int * n_frames)()
        n = C.c_int()
        keep, Kp, dpp, nd = _camera(K, dist) if K is not None else (None, None, None, 0)
        check(self._L.asl_detect_batch_device(self._h, _ptr(data_ptr), n_frames, channels, width, height, stride, frame_pitch,
                                              _ptr(stream), Kp, dpp, nd, float(tag_size), out.ctypes.data,
                                              poses.ctypes.data if want_poses else None, cap, npf, C.byref(n)))
        if n.value > cap:
            return self.detect_device(data_ptr, n_frames, channels, width, height, stride, frame_pitch, stream, K, dist,
                                      tag_size, max_per_frame=(n.value + n_frames - 1) // n_frames + 1, want_poses=want_poses,
                                      reuse_buffers=reuse_buffers)
        return out[:n.value], (poses[:n.value] if want_poses else None), np.array(list(npf), dtype=np.int64)

    def submit_device(self, data_ptr, n_frames, channels, width, height, stride=None, frame_pitch=None, stream=0, K=None,
                      dist=None, tag_size=0.0):
        """Enqueue a batch resident in HBM and return immediately (asl_submit_batch_device); pair with collect()."""
        stride = stride or width * channels
        frame_pitch = frame_pitch or stride * height
        keep, Kp, dpp, nd = _camera(K, dist) if K is not None else (None, None, None, 0)
        check(self._L.asl_submit_batch_device(self._h, _ptr(data_ptr), n_frames, channels, width, height, stride, frame_pitch,
                                              _ptr(stream), Kp, dpp, nd, float(tag_size)))
        self._inflight = (n_frames, K is not None)

    def render_frames_device(self, frames_ptr, n_frames, width, height, planes_ptr, max_planes, textures_ptr, tw, th, half, K=None, dist=None,
                             stride=None, frame_pitch=None, stream=0):
        """asl_render_frames_device: BGR frames straight into device memory (frames_ptr, planes_ptr, textures_ptr are device
        addresses; K / dist are host arrays, only for a camera with lens distortion)."""
        stride = stride or 3 * width
        frame_pitch = frame_pitch or stride * height
        Kp = dpp = None
        nd = 0
        if dist is not None:
            Kc = np.ascontiguousarray(K, dtype=np.float64)
            dc = np.ascontiguousarray(dist, dtype=np.float64).ravel()
            Kp, dpp, nd = Kc.ctypes.data_as(_DP), dc.ctypes.data_as(_DP), len(dc)
        check(self._L.asl_render_frames_device(self._h, _ptr(frames_ptr), int(n_frames), int(width), int(height), int(stride),
                                               int(frame_pitch), _ptr(planes_ptr), int(max_planes), _ptr(textures_ptr),
                                               int(tw), int(th), float(half), Kp, dpp, nd, _ptr(stream)))

    def rectify_frames_device(self, src_ptr, n_frames, channels, width, height, dst_ptr, K, dist, K_new=None, width_out=None,
                              height_out=None, fill=0, stride=None, frame_pitch=None, stride_out=None, frame_pitch_out=None, stream=0):
        """asl_rectify_frames_device: n_frames gray / BGR frames of the camera (K, dist) at the device address src_ptr -> the
        gray frames of the pinhole K_new (default K) at dst_ptr, width_out x height_out (default: the source's size);
        enqueued on `stream`, no wait.  K, dist and K_new are host arrays."""
        width_out, height_out = int(width_out or width), int(height_out or height)
        stride = stride or width * channels
        frame_pitch = frame_pitch or stride * height
        stride_out = stride_out or width_out
        frame_pitch_out = frame_pitch_out or stride_out * height_out
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        Kn = None if K_new is None else np.ascontiguousarray(K_new, dtype=np.float64)
        if Kn is not None and Kn.shape != (3, 3):
            raise ValueError("K_new must be 3x3")
        check(self._L.asl_rectify_frames_device(self._h, _ptr(src_ptr), int(n_frames), int(channels), int(width), int(height), int(stride),
                                                int(frame_pitch), _ptr(dst_ptr), width_out, height_out, int(stride_out), int(frame_pitch_out),
                                                Kp, dpp, nd, None if Kn is None else Kn.ctypes.data_as(_DP), int(fill), _ptr(stream)))

    def rectify(self, image, K, dist, K_new=None, size=None, fill=0):
        """asl_rectify_u8: one host image, (H, W) gray or (H, W, 3) BGR uint8, of the camera (K, dist) -> the (h_out, w_out)
        gray image of the pinhole K_new (default K); size = (w_out, h_out), default the source's."""
        a = np.ascontiguousarray(image)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("expected an (H, W) or (H, W, 3) uint8 image")
        h, w = a.shape[:2]
        ch = 1 if a.ndim == 2 else 3
        w_out, h_out = (w, h) if size is None else (int(size[0]), int(size[1]))
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        Kn = None if K_new is None else np.ascontiguousarray(K_new, dtype=np.float64)
        if Kn is not None and Kn.shape != (3, 3):
            raise ValueError("K_new must be 3x3")
        out = np.empty((max(h_out, 0), max(w_out, 0)), dtype=np.uint8)
        check(self._L.asl_rectify_u8(self._h, a.ctypes.data, ch, w, h, w * ch, out.ctypes.data, w_out, h_out, w_out, Kp, dpp, nd,
                                     None if Kn is None else Kn.ctypes.data_as(_DP), int(fill)))
        return out

    def rectify_views_device(self, src_ptr, n_frames, channels, width, height, dst_ptr, K, dist, views, model="fisheye", width_out=None,
                             height_out=None, theta_max=None, fill=0, stride=None, frame_pitch=None, stride_out=None, frame_pitch_out=None,
                             stream=0):
        """asl_rectify_views_device: n_frames gray / BGR frames of the camera (K, dist, model) at the device address src_ptr
        -> the gray frames of the rotated pinholes `views` ([(K_new, R)], R = source camera <- view, or RECTIFY_VIEW_DTYPE
        records) at dst_ptr, view-major: view v of frame i at dst_ptr + (v * n_frames + i) * frame_pitch_out.  theta_max
        (radians, None = pi): fisheye rays further from the axis give `fill`.  Enqueued on `stream`, no wait."""
        width_out, height_out = int(width_out or width), int(height_out or height)
        stride = stride or width * channels
        frame_pitch = frame_pitch or stride * height
        stride_out = stride_out or width_out
        frame_pitch_out = frame_pitch_out or stride_out * height_out
        keep, Kp, dpp, nd, m = _lens(K, dist, model)
        rec = rectify_view_records(views)
        check(self._L.asl_rectify_views_device(self._h, _ptr(src_ptr), int(n_frames), int(channels), int(width), int(height), int(stride),
                                               int(frame_pitch), _ptr(dst_ptr), width_out, height_out, int(stride_out), int(frame_pitch_out),
                                               Kp, dpp, nd, m, _data(rec), len(rec), float(theta_max or 0.0), int(fill), _ptr(stream)))

    def rectify_views(self, image, K, dist, views, model="fisheye", size=None, theta_max=None, fill=0):
        """asl_rectify_views_u8: one host image, (H, W) gray or (H, W, 3) BGR uint8, of the camera (K, dist, model) -> the
        (n_views, h_out, w_out) gray images of the rotated pinholes `views`; size = (w_out, h_out), default the source's."""
        a = np.ascontiguousarray(image)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("expected an (H, W) or (H, W, 3) uint8 image")
        h, w = a.shape[:2]
        ch = 1 if a.ndim == 2 else 3
        w_out, h_out = (w, h) if size is None else (int(size[0]), int(size[1]))
        keep, Kp, dpp, nd, m = _lens(K, dist, model)
        rec = rectify_view_records(views)
        out = np.empty((len(rec), max(h_out, 0), max(w_out, 0)), dtype=np.uint8)
        check(self._L.asl_rectify_views_u8(self._h, a.ctypes.data, ch, w, h, w * ch, out.ctypes.data, w_out, h_out, w_out, max(w_out * h_out, 0),
                                           Kp, dpp, nd, m, _data(rec), len(rec), float(theta_max or 0.0), int(fill)))
        return out

    def pack_observations_device(self, out_ptr, max_tags, stream=0):
        """asl_pack_observations_device: the submitted batch's results as n_frames x max_tags asl_obs records at the
        device address `out_ptr`, enqueued on `stream` (use the stream the batch was submitted on)."""
        check(self._L.asl_pack_observations_device(self._h, _ptr(out_ptr), int(max_tags), _ptr(stream)))

    def graph_frames_device(self, obs_ptr, world, n_frames, max_tags, coordinate_id, pose_ptr, status_ptr, last_ptr, n_ids, picks_ptr=0,
                            stream=0):
        """asl_graph_frames_device (all pointers are device addresses; picks_ptr = 0 skips the picks)."""
        check(self._L.asl_graph_frames_device(self._h, _ptr(obs_ptr), int(world), int(n_frames), int(max_tags), int(coordinate_id),
                                              _ptr(pose_ptr), _ptr(status_ptr), _ptr(last_ptr), int(n_ids), _opt_ptr(picks_ptr),
                                              _ptr(stream)))

    def graph_picks_device(self, obs_ptr, world, n_frames, max_tags, status_ptr, order_lo, order_hi, last_ptr, n_ids, picks_ptr, stream=0):
        """asl_graph_picks_device: last sightings + picks of the status-0 frames at positions [order_lo, order_hi)."""
        check(self._L.asl_graph_picks_device(self._h, _ptr(obs_ptr), int(world), int(n_frames), int(max_tags), _ptr(status_ptr),
                                             int(order_lo), int(order_hi), _ptr(last_ptr), int(n_ids), _ptr(picks_ptr), _ptr(stream)))

    def localize(self, obs, tag_map, K, dist, tag_size, max_tag_rms_px=0.0, sigma_px=None, map_cov=None):
        """asl_localize_batch: host records obs (n_frames, max_tags) OBS_DTYPE (e.g. dist.pack_observations) against
        tag_map (n_ids,) MAP_TAG_DTYPE (or a localize.TagMap) -> (n_frames,) CAM_POSE_DTYPE, world<-camera per frame.
        sigma_px not None: asl_localize_cov_batch -> (poses, (n_frames,) POSE_COV_DTYPE), the covariance scaled by that
        corner sigma, or by the solve's own estimate for 0.
        tag_size is the size of the map entries whose size is 0; an entry with a size of its own (TagMap.set_size) is solved at it.
        map_cov (a mapping.MapCovariance, or (cov_slot, matrix) as build_map(with_cov=True) returns them; with sigma_px):
        asl_localize_mapcov_batch -- the uncertainty of the map's tags is carried into the covariances."""
        if map_cov is not None and sigma_px is None:
            raise ValueError("map_cov needs the covariance form: give sigma_px (0: estimated from the solve)")
        o, m = _obs_records(obs), _map_records(tag_map)
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        out = np.zeros(o.shape[0], dtype=CAM_POSE_DTYPE)
        args = (self._h, _data(o), o.shape[0], o.shape[1], _data(m), len(m), Kp, dpp, nd, float(tag_size), float(max_tag_rms_px))
        if sigma_px is None:
            check(self._L.asl_localize_batch(*args, _data(out)))
            return out
        cov = np.zeros(o.shape[0], dtype=POSE_COV_DTYPE)
        if map_cov is not None:
            slot, mat, ld = _map_cov_args(map_cov, len(m))
            check(self._L.asl_localize_mapcov_batch(*args, float(sigma_px), _data(out), _data(cov), mat.ctypes.data, ld, slot.ctypes.data))
            return out, cov
        check(self._L.asl_localize_cov_batch(*args, float(sigma_px), _data(out), _data(cov)))
        return out, cov

    def localize_device(self, obs_ptr, n_frames, max_tags, map_ptr, n_ids, out_ptr, K, dist, tag_size, max_tag_rms_px=0.0,
                        stream=0, cov_ptr=None, sigma_px=0.0, map_cov=None):
        """asl_localize_frames_device: obs_ptr (n_frames x max_tags asl_obs, e.g. from pack_observations_device), map_ptr
        (n_ids asl_map_tag) and out_ptr (n_frames asl_cam_pose) are device addresses; enqueued on `stream`, no wait.
        cov_ptr not None (n_frames asl_pose_cov): asl_localize_cov_frames_device with sigma_px.  map_cov, (map_cov_ptr, ld,
        cov_slot_ptr) as build_map_device's cov wrote them (ld = 6 cap_tags), with cov_ptr: asl_localize_mapcov_frames_device."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        args = (self._h, _ptr(obs_ptr), int(n_frames), int(max_tags), _ptr(map_ptr), int(n_ids), Kp, dpp, nd, float(tag_size), float(max_tag_rms_px))
        if map_cov is not None:
            check(self._L.asl_localize_mapcov_frames_device(*args, float(sigma_px), _ptr(out_ptr), _opt_ptr(cov_ptr), _opt_ptr(map_cov[0]), int(map_cov[1]),
                                                            _opt_ptr(map_cov[2]), _ptr(stream)))
        elif cov_ptr is None:
            check(self._L.asl_localize_frames_device(*args, _ptr(out_ptr), _ptr(stream)))
        else:
            check(self._L.asl_localize_cov_frames_device(*args, float(sigma_px), _ptr(out_ptr), _ptr(cov_ptr), _ptr(stream)))

    def localize_rig(self, obs, tag_map, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None, map_cov=None):
        """asl_localize_rig_batch: host records obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, against tag_map and
        the camera table rig ((n_cams,) RIG_CAMERA_DTYPE, or a rig.Rig) -> (n_frames,) CAM_POSE_DTYPE, world<-rig per frame.
        sigma_px not None: asl_localize_rig_cov_batch -> (poses, (n_frames,) POSE_COV_DTYPE), as localize.
        tag_size is the size of the map entries whose size is 0, as in localize.  map_cov as in localize:
        asl_localize_rig_mapcov_batch."""
        if map_cov is not None and sigma_px is None:
            raise ValueError("map_cov needs the covariance form: give sigma_px (0: estimated from the solve)")
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        m = _map_records(tag_map)
        r = _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        out = np.zeros(o.shape[1], dtype=CAM_POSE_DTYPE)
        args = (self._h, _data(o), o.shape[0], o.shape[1], o.shape[2], _data(m), len(m), _data(r), float(tag_size), float(max_tag_rms_px))
        if sigma_px is None:
            check(self._L.asl_localize_rig_batch(*args, _data(out)))
            return out
        cov = np.zeros(o.shape[1], dtype=POSE_COV_DTYPE)
        if map_cov is not None:
            slot, mat, ld = _map_cov_args(map_cov, len(m))
            check(self._L.asl_localize_rig_mapcov_batch(*args, float(sigma_px), _data(out), _data(cov), mat.ctypes.data, ld, slot.ctypes.data))
            return out, cov
        check(self._L.asl_localize_rig_cov_batch(*args, float(sigma_px), _data(out), _data(cov)))
        return out, cov

    def localize_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, map_ptr, n_ids, rig_ptr, out_ptr, tag_size, max_tag_rms_px=0.0,
                            stream=0, cov_ptr=None, sigma_px=0.0, map_cov=None):
        """asl_localize_rig_frames_device: obs_ptr (n_cams x n_frames x max_tags asl_obs, camera-major), map_ptr (n_ids
        asl_map_tag), rig_ptr (n_cams asl_rig_camera, complete when the call is made) and out_ptr (n_frames asl_cam_pose) are
        device addresses; enqueued on `stream`.  cov_ptr not None (n_frames asl_pose_cov): asl_localize_rig_cov_frames_device.
        map_cov as in localize_device: asl_localize_rig_mapcov_frames_device."""
        args = (self._h, _ptr(obs_ptr), int(n_cams), int(n_frames), int(max_tags), _ptr(map_ptr), int(n_ids), _ptr(rig_ptr), float(tag_size),
                float(max_tag_rms_px))
        if map_cov is not None:
            check(self._L.asl_localize_rig_mapcov_frames_device(*args, float(sigma_px), _ptr(out_ptr), _opt_ptr(cov_ptr), _opt_ptr(map_cov[0]),
                                                                int(map_cov[1]), _opt_ptr(map_cov[2]), _ptr(stream)))
        elif cov_ptr is None:
            check(self._L.asl_localize_rig_frames_device(*args, _ptr(out_ptr), _ptr(stream)))
        else:
            check(self._L.asl_localize_rig_cov_frames_device(*args, float(sigma_px), _ptr(out_ptr), _ptr(cov_ptr), _ptr(stream)))

    def localize_bundles(self, obs, bundles, K, dist, tag_size, max_tag_rms_px=0.0, sigma_px=None):
        """asl_localize_bundles_batch: host records obs (n_frames, max_tags) OBS_DTYPE against bundles (a bundles.BundleSet, or
        (n_bundles, n_ids) MAP_TAG_DTYPE tables, bundle<-tag) -> (n_frames, n_bundles) CAM_POSE_DTYPE with T = bundle<-camera,
        entry [f, b] what localize gives for frame f with table b as its map, to the byte.  sigma_px not None: (poses,
        (n_frames, n_bundles) POSE_COV_DTYPE), as localize."""
        o, t = _obs_records(obs), _bundle_tables(bundles)
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        shape = (o.shape[0], t.shape[0])
        out = np.zeros(shape, dtype=CAM_POSE_DTYPE)
        cov = np.zeros(shape, dtype=POSE_COV_DTYPE) if sigma_px is not None else None
        check(self._L.asl_localize_bundles_batch(self._h, _data(o), o.shape[0], o.shape[1], _data(t), t.shape[0], t.shape[1], Kp, dpp, nd, float(tag_size),
                                                 float(max_tag_rms_px), float(sigma_px or 0.0), _data(out), None if cov is None else _data(cov)))
        return out if cov is None else (out, cov)

    def localize_bundles_device(self, obs_ptr, n_frames, max_tags, maps_ptr, n_bundles, n_ids, out_ptr, K, dist, tag_size, max_tag_rms_px=0.0,
                                stream=0, cov_ptr=None, sigma_px=0.0):
        """asl_localize_bundles_frames_device: localize_device with maps_ptr (n_bundles x n_ids asl_map_tag) in place of the
        map and n_frames x n_bundles records at out_ptr and, if not None, cov_ptr; enqueued on `stream`, no wait."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        check(self._L.asl_localize_bundles_frames_device(self._h, _ptr(obs_ptr), int(n_frames), int(max_tags), _ptr(maps_ptr), int(n_bundles), int(n_ids),
                                                         Kp, dpp, nd, float(tag_size), float(max_tag_rms_px), float(sigma_px), _ptr(out_ptr),
                                                         _opt_ptr(cov_ptr), _ptr(stream)))

    def localize_bundles_rig(self, obs, bundles, rig, tag_size, max_tag_rms_px=0.0, sigma_px=None):
        """asl_localize_bundles_rig_batch: localize_bundles for a rig's block obs (n_cams, n_frames, max_tags), camera-major ->
        (n_frames, n_bundles) CAM_POSE_DTYPE with T = bundle<-rig, entry [f, b] what localize_rig gives with table b."""
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        t, r = _bundle_tables(bundles), _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        shape = (o.shape[1], t.shape[0])
        out = np.zeros(shape, dtype=CAM_POSE_DTYPE)
        cov = np.zeros(shape, dtype=POSE_COV_DTYPE) if sigma_px is not None else None
        check(self._L.asl_localize_bundles_rig_batch(self._h, _data(o), o.shape[0], o.shape[1], o.shape[2], _data(t), t.shape[0], t.shape[1], _data(r),
                                                     float(tag_size), float(max_tag_rms_px), float(sigma_px or 0.0), _data(out),
                                                     None if cov is None else _data(cov)))
        return out if cov is None else (out, cov)

    def localize_bundles_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, maps_ptr, n_bundles, n_ids, rig_ptr, out_ptr, tag_size,
                                    max_tag_rms_px=0.0, stream=0, cov_ptr=None, sigma_px=0.0):
        """asl_localize_bundles_rig_frames_device: localize_rig_device with maps_ptr (n_bundles x n_ids asl_map_tag) in place of
        the map and n_frames x n_bundles records at out_ptr and, if not None, cov_ptr; enqueued on `stream`."""
        check(self._L.asl_localize_bundles_rig_frames_device(self._h, _ptr(obs_ptr), int(n_cams), int(n_frames), int(max_tags), _ptr(maps_ptr),
                                                             int(n_bundles), int(n_ids), _ptr(rig_ptr), float(tag_size), float(max_tag_rms_px),
                                                             float(sigma_px), _ptr(out_ptr), _opt_ptr(cov_ptr), _ptr(stream)))

    def bundle_relative(self, poses, cov, ref):
        """asl_bundle_relative_batch: poses (n_frames, n_bundles) CAM_POSE_DTYPE as localize_bundles returns them, cov their
        (n_frames, n_bundles) POSE_COV_DTYPE or None -> (n_frames, n_bundles) BUNDLE_REL_DTYPE, T = ref<-bundle with its
        covariance (status 2, zeros, without cov).  The two poses of a pair are taken as independent."""
        p = np.ascontiguousarray(poses, dtype=CAM_POSE_DTYPE)
        if p.ndim != 2:
            raise ValueError("poses must be (n_frames, n_bundles) asl_cam_pose records")
        c = None if cov is None else np.ascontiguousarray(cov, dtype=POSE_COV_DTYPE)
        if c is not None and c.shape != p.shape:
            raise ValueError("cov must have the shape of poses")
        rel = np.zeros(p.shape, dtype=BUNDLE_REL_DTYPE)
        check(self._L.asl_bundle_relative_batch(self._h, _data(p), None if c is None else _data(c), p.shape[0], p.shape[1], int(ref), _data(rel)))
        return rel

    def bundle_relative_device(self, poses_ptr, cov_ptr, n_frames, n_bundles, ref, rel_ptr, stream=0):
        """asl_bundle_relative_device: poses_ptr (n_frames x n_bundles asl_cam_pose), cov_ptr (as many asl_pose_cov, or None)
        and rel_ptr (as many asl_bundle_rel) are device addresses; enqueued on `stream`, no wait."""
        check(self._L.asl_bundle_relative_device(self._h, _ptr(poses_ptr), _opt_ptr(cov_ptr), int(n_frames), int(n_bundles), int(ref), _ptr(rel_ptr),
                                                 _ptr(stream)))

    def locate_tags(self, obs, poses, map_records, K, dist, tag_size, max_view_rms_px=0.0, min_views=2, sigma_px=None):
        """asl_locate_tags_batch: host records obs (n_frames, max_tags) OBS_DTYPE, their frames' poses (n_frames,)
        CAM_POSE_DTYPE (world<-camera: what localize, smooth or build_map return) and a map block (n_ids,) MAP_TAG_DTYPE (or a
        localize.TagMap) -> (the extended map, (n_ids,) TAG_FIT_DTYPE, (n_ids,) POSE_COV_DTYPE or None).  Every id whose
        entry has valid == 0 (and a size that is 0, the call's tag_size, or the tag's own side) is solved from all its
        views with the cameras held fixed; a located tag's entry gets its pose and valid = 1, every other entry keeps its
        bytes.  The caller's array is not modified.  max_view_rms_px > 0: the outlier gate on single views.  sigma_px not
        None: also the covariance of every located world<-tag, scaled by that corner sigma, or by the solve's own
        estimate for 0."""
        o, m = _obs_records(obs), _map_records(map_records).copy()
        p = np.ascontiguousarray(poses, dtype=CAM_POSE_DTYPE).ravel()
        if len(p) != o.shape[0]:
            raise ValueError("one pose per frame: obs has %d frames, poses %d" % (o.shape[0], len(p)))
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        fit = np.zeros(len(m), dtype=TAG_FIT_DTYPE)
        cov = np.zeros(len(m), dtype=POSE_COV_DTYPE) if sigma_px is not None else None
        none = np.zeros(1, dtype=CAM_POSE_DTYPE)   # no frame: the block and the poses are never read, but must not be NULL
        check(self._L.asl_locate_tags_batch(self._h, _data(o) or none.ctypes.data, o.shape[0], o.shape[1], _data(p) or none.ctypes.data, _data(m),
                                            len(m), Kp, dpp, nd, float(tag_size), float(max_view_rms_px), int(min_views),
                                            float(sigma_px or 0.0), _data(fit), None if cov is None else _data(cov)))
        return m, fit, cov

    def locate_tags_device(self, obs_ptr, n_frames, max_tags, poses_ptr, map_ptr, n_ids, fit_ptr, K, dist, tag_size, max_view_rms_px=0.0,
                           min_views=2, stream=0, cov_ptr=None, sigma_px=0.0):
        """asl_locate_tags_frames_device: obs_ptr (n_frames x max_tags asl_obs), poses_ptr (n_frames asl_cam_pose), map_ptr
        (n_ids asl_map_tag, read and written in place), fit_ptr (n_ids asl_tag_fit) and cov_ptr (n_ids asl_pose_cov, or None)
        are device addresses; enqueued on `stream`, no wait."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        check(self._L.asl_locate_tags_frames_device(self._h, _ptr(obs_ptr), int(n_frames), int(max_tags), _ptr(poses_ptr), _ptr(map_ptr), int(n_ids),
                                                    Kp, dpp, nd, float(tag_size), float(max_view_rms_px), int(min_views), float(sigma_px),
                                                    _ptr(fit_ptr), _opt_ptr(cov_ptr), _ptr(stream)))

    def locate_tags_rig(self, obs, poses, tag_map, rig, tag_size, max_view_rms_px=0.0, min_views=2, sigma_px=None):
        """asl_locate_tags_rig_batch: locate_tags for a rig.  Host records obs (n_cams, n_frames, max_tags) OBS_DTYPE,
        camera-major, the frames' poses (n_frames,) CAM_POSE_DTYPE with T = world<-rig (what localize_rig, smooth_rig or
        build_map_rig return), a map block (or a localize.TagMap) and the camera table rig ((n_cams,) RIG_CAMERA_DTYPE, or a
        rig.Rig) -> (the extended map, (n_ids,) TAG_FIT_DTYPE, (n_ids,) POSE_COV_DTYPE or None).  Every camera's view of a
        tag in a frame is a view of its own, through that camera's model and mounting.  The caller's block is not modified."""
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        m, r = _map_records(tag_map).copy(), _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        p = np.ascontiguousarray(poses, dtype=CAM_POSE_DTYPE).ravel()
        if len(p) != o.shape[1]:
            raise ValueError("one pose per frame: obs has %d frames, poses %d" % (o.shape[1], len(p)))
        fit = np.zeros(len(m), dtype=TAG_FIT_DTYPE)
        cov = np.zeros(len(m), dtype=POSE_COV_DTYPE) if sigma_px is not None else None
        none = np.zeros(1, dtype=CAM_POSE_DTYPE)   # no frame: the block and the poses are never read, but must not be NULL
        check(self._L.asl_locate_tags_rig_batch(self._h, _data(o) or none.ctypes.data, o.shape[0], o.shape[1], o.shape[2],
                                                _data(p) or none.ctypes.data, _data(m), len(m), _data(r), float(tag_size), float(max_view_rms_px),
                                                int(min_views), float(sigma_px or 0.0), _data(fit), None if cov is None else _data(cov)))
        return m, fit, cov

    def locate_tags_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, poses_ptr, map_ptr, n_ids, rig_ptr, fit_ptr, tag_size,
                               max_view_rms_px=0.0, min_views=2, stream=0, cov_ptr=None, sigma_px=0.0):
        """asl_locate_tags_rig_frames_device: obs_ptr (n_cams x n_frames x max_tags asl_obs, camera-major), poses_ptr (n_frames
        asl_cam_pose, world<-rig), map_ptr (n_ids asl_map_tag, read and written in place), rig_ptr (n_cams asl_rig_camera,
        complete when the call is made), fit_ptr (n_ids asl_tag_fit) and cov_ptr (n_ids asl_pose_cov, or None) are device
        addresses; enqueued on `stream`, no wait."""
        check(self._L.asl_locate_tags_rig_frames_device(self._h, _ptr(obs_ptr), int(n_cams), int(n_frames), int(max_tags), _ptr(poses_ptr),
                                                        _ptr(map_ptr), int(n_ids), _ptr(rig_ptr), float(tag_size), float(max_view_rms_px),
                                                        int(min_views), float(sigma_px), _ptr(fit_ptr), _opt_ptr(cov_ptr), _ptr(stream)))

    def pose_cov(self, corners, T, K, dist, tag_size, sigma_px=0.0):
        """asl_solve_pnp_cov_batch: the covariance of the camera<-tag poses T (N, 4, 4) that solve_pnp returned for corners
        (N, 4, 2) -> (N,) POSE_COV_DTYPE; a T with non-finite entries (a failed PnP) gets status 1."""
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 4, 2))
        Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(-1, 16))
        if len(Tc) != len(c):
            raise ValueError("one 4x4 pose per 4 corners")
        keep, Kp, dpp, nd = _camera(K, dist)
        cov = np.zeros(len(c), dtype=POSE_COV_DTYPE)
        check(self._L.asl_solve_pnp_cov_batch(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), Tc.ctypes.data_as(_DP), Kp, dpp, nd, float(tag_size),
                                              float(sigma_px), _data(cov), len(c)))
        return cov

    def pose_cov_device(self, obs_ptr, n_records, cov_ptr, K, dist, tag_size, sigma_px=0.0, stream=0):
        """asl_pose_cov_device: obs_ptr (n_records asl_obs, e.g. a pack_observations_device block) and cov_ptr (n_records
        asl_pose_cov) are device addresses; enqueued on `stream`, no wait."""
        keep, Kp, dpp, nd = _camera(K, dist)
        check(self._L.asl_pose_cov_device(self._h, _ptr(obs_ptr), int(n_records), Kp, dpp, nd, float(tag_size), float(sigma_px), _ptr(cov_ptr),
                                          _ptr(stream)))

    @staticmethod
    def _calib_args(K_init, n_dist, model=None):
        """(array to keep alive, K_init pointer or None, lens_model or None: the call without a lens)"""
        m = None
        if model is not None:
            m = LENS_MODELS.get(model, model)
            if m not in (LENS_BROWN, LENS_FISHEYE):
                raise ValueError("model must be 'brown' or 'fisheye'")
        if m == LENS_FISHEYE:
            if int(n_dist) not in (0, 4):
                raise ValueError("a fisheye lens has 0 or 4 coefficients (k1, k2, k3, k4)")
        elif int(n_dist) not in (0, 4, 5):
            raise ValueError("n_dist must be 0, 4 or 5")
        if K_init is None:
            return None, None, m
        Kc = np.ascontiguousarray(K_init, dtype=np.float64)
        if Kc.shape != (3, 3):
            raise ValueError("K_init must be 3x3")
        return Kc, Kc.ctypes.data_as(_DP), m

    def calibrate(self, obs, tag_map, tag_size, width, height, K_init=None, n_dist=5, flags=0, max_iters=30, model=None):
        """asl_calibrate_batch: host records obs (n_frames, max_tags) OBS_DTYPE of a target whose tag poses tag_map
        ((n_ids,) MAP_TAG_DTYPE or a localize.TagMap) gives -> (CALIB_RESULT_DTYPE record, (n_frames,) CAM_POSE_DTYPE).
        tag_size is the size of the map entries whose size is 0: a target may mix tags of several sizes (TagMap.set_size).
        model: "brown" or "fisheye" (n_dist 0 or 4: dist = k1 k2 k3 k4, from the corners of the RAW frames), through
        asl_calibrate_lens_batch; None is the call without a lens, the Brown model."""
        o, m = _obs_records(obs), _map_records(tag_map)
        keep, Kp, lens = self._calib_args(K_init, n_dist, model)
        res = np.zeros((), dtype=CALIB_RESULT_DTYPE)
        poses = np.zeros(o.shape[0], dtype=CAM_POSE_DTYPE)
        head = (self._h, _data(o), o.shape[0], o.shape[1], _data(m), len(m), float(tag_size), int(width), int(height), Kp)
        tail = (int(n_dist), int(flags), int(max_iters), res.ctypes.data, _data(poses))
        check(self._L.asl_calibrate_batch(*head, *tail) if lens is None else self._L.asl_calibrate_lens_batch(*head, lens, *tail))
        return res, poses

    def calibrate_device(self, obs_ptr, n_frames, max_tags, map_ptr, n_ids, tag_size, width, height, result_ptr, poses_ptr,
                         K_init=None, n_dist=5, flags=0, max_iters=30, stream=0, model=None):
        """asl_calibrate_frames_device: obs_ptr (n_frames x max_tags asl_obs), map_ptr (n_ids asl_map_tag), result_ptr (one
        asl_calib_result) and poses_ptr (n_frames asl_cam_pose) are device addresses; the whole solve is enqueued on
        `stream`, no wait.  model as in calibrate (asl_calibrate_lens_frames_device)."""
        keep, Kp, lens = self._calib_args(K_init, n_dist, model)
        head = (self._h, _ptr(obs_ptr), int(n_frames), int(max_tags), _ptr(map_ptr), int(n_ids), float(tag_size), int(width), int(height), Kp)
        tail = (int(n_dist), int(flags), int(max_iters), _ptr(result_ptr), _ptr(poses_ptr), _ptr(stream))
        check(self._L.asl_calibrate_frames_device(*head, *tail) if lens is None else self._L.asl_calibrate_lens_frames_device(*head, lens, *tail))

    def calibrate_rig(self, obs, tag_map, rig, tag_size, max_iters=30, sigma_px=None):
        """asl_calibrate_rig_batch: host records obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, against tag_map, with
        rig ((n_cams,) RIG_CAMERA_DTYPE, or a rig.Rig) as the initial mountings -> ((n_cams,) RIG_CAMERA_DTYPE with the refined
        mountings, RIG_CALIB_RESULT_DTYPE record, (n_cams,) POSE_COV_DTYPE of the mountings, (n_frames,) CAM_POSE_DTYPE
        world<-rig).  Camera 0's mounting is the gauge and stays; sigma_px None or 0: the covariances are scaled by the
        solve's own estimate.  Pass clean observations: the joint solve has no outlier gate."""
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        m, r = _map_records(tag_map), _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        rig_out = np.zeros(len(r), dtype=RIG_CAMERA_DTYPE)
        res = np.zeros((), dtype=RIG_CALIB_RESULT_DTYPE)
        cov = np.zeros(len(r), dtype=POSE_COV_DTYPE)
        poses = np.zeros(o.shape[1], dtype=CAM_POSE_DTYPE)
        check(self._L.asl_calibrate_rig_batch(self._h, _data(o), o.shape[0], o.shape[1], o.shape[2], _data(m), len(m), _data(r), float(tag_size),
                                              int(max_iters), float(sigma_px or 0.0), _data(rig_out), res.ctypes.data, _data(cov), _data(poses)))
        return rig_out, res, cov, poses

    def calibrate_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, map_ptr, n_ids, rig_ptr, tag_size, rig_out_ptr, result_ptr, cov_ptr,
                             poses_ptr, max_iters=30, sigma_px=0.0, stream=0):
        """asl_calibrate_rig_frames_device: obs_ptr (n_cams x n_frames x max_tags asl_obs, camera-major), map_ptr (n_ids
        asl_map_tag), rig_ptr (n_cams asl_rig_camera, complete when the call is made), rig_out_ptr (n_cams asl_rig_camera; may
        be rig_ptr), result_ptr (one asl_rig_calib_result), cov_ptr (n_cams asl_pose_cov) and poses_ptr (n_frames asl_cam_pose)
        are device addresses; the whole solve is enqueued on `stream`, no wait."""
        check(self._L.asl_calibrate_rig_frames_device(self._h, _ptr(obs_ptr), int(n_cams), int(n_frames), int(max_tags), _ptr(map_ptr), int(n_ids),
                                                      _ptr(rig_ptr), float(tag_size), int(max_iters), float(sigma_px), _ptr(rig_out_ptr),
                                                      _ptr(result_ptr), _ptr(cov_ptr), _ptr(poses_ptr), _ptr(stream)))

    def build_map(self, obs, n_ids, K, dist, tag_size, world_id=-1, max_iters=30, with_std=True, huber_px=0.0, with_slot_weight=False,
                  tag_sizes=None, with_cov=False):
        """asl_map_batch: host records obs (n_frames, max_tags) OBS_DTYPE that see an unknown set of tags -> (MAP_RESULT_DTYPE
        record, (n_ids,) MAP_TAG_DTYPE world<-tag map, (n_ids, 6) tag std or None, (n_frames,) CAM_POSE_DTYPE world<-camera).
        huber_px > 0 or with_slot_weight: asl_map_robust_batch -- a Huber loss of that many pixels on every corner residual of
        the joint LM (0: the plain computation); the result's n_soft counts the down-weighted observations.
        with_slot_weight: a fifth item, (n_frames, max_tags) doubles: a slot's smallest corner weight, 0 outside the solve.
        tag_sizes ({id: size} or n_ids sizes; 0: tag_size): asl_map_sized_batch -- tags of different known sizes, each solved
        at its own and returned with it in the map's size field.
        with_cov: asl_mapcov_batch -- a last item (cov_slot (n_ids,) int32, matrix): the joint covariance of the mapped tags
        other than the world tag, block cov_slot[id] of the 6 n_cov x 6 n_cov matrix (mapping.MapCovariance wraps the pair)."""
        o = _obs_records(obs)
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        return self._map_host(o, o.shape[0], n_ids, [o.shape[0], o.shape[1]], [Kp, dpp, nd], False, tag_size, tag_sizes, world_id, huber_px,
                              max_iters, with_std, with_slot_weight, with_cov)

    def build_map_device(self, obs_ptr, n_frames, max_tags, n_ids, K, dist, tag_size, map_ptr, std_ptr, poses_ptr, result_ptr,
                         world_id=-1, max_iters=30, stream=0, huber_px=0.0, slot_weight_ptr=0, tag_sizes=None, cov=None):
        """asl_map_frames_device: obs_ptr (n_frames x max_tags asl_obs, e.g. from pack_observations_device), map_ptr (n_ids
        asl_map_tag, out), std_ptr (n_ids x 6 doubles or 0), poses_ptr (n_frames asl_cam_pose) and result_ptr (one
        asl_map_result) are device addresses; enqueued on `stream` after one wait for the problem size.
        huber_px > 0 or slot_weight_ptr (n_frames x max_tags doubles): asl_map_robust_frames_device.
        tag_sizes ({id: size} or n_ids sizes, on the host): asl_map_sized_frames_device.
        cov, (cov_slot_ptr (n_ids int32), map_cov_ptr (6 cap_tags x 6 cap_tags doubles), cap_tags): asl_mapcov_frames_device."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        self._map_call(True, obs_ptr, [int(n_frames), int(max_tags)], n_ids, [Kp, dpp, nd], False, tag_size, tag_sizes, world_id, huber_px, max_iters,
                       (map_ptr, std_ptr, poses_ptr, result_ptr), slot_weight_ptr, stream, cov)

    def build_map_rig(self, obs, n_ids, rig, tag_size, world_id=-1, max_iters=30, with_std=True, huber_px=0.0, with_slot_weight=False,
                      tag_sizes=None, with_cov=False):
        """asl_map_rig_batch: host records obs (n_cams, n_frames, max_tags) OBS_DTYPE, camera-major, of a rig whose camera table
        is rig ((n_cams,) RIG_CAMERA_DTYPE, or a rig.Rig) -> build_map's items with poses = world<-rig per frame; huber_px as
        there (0: the squared loss).  with_slot_weight: a fifth item, (n_cams, n_frames, max_tags) doubles.  tag_sizes as
        there: asl_map_rig_sized_batch.  with_cov as there: asl_mapcov_rig_batch."""
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        r = _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        return self._map_host(o, o.shape[1], n_ids, list(o.shape), [_data(r)], True, tag_size, tag_sizes, world_id, huber_px, max_iters, with_std,
                              with_slot_weight, with_cov)

    def build_map_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, n_ids, rig_ptr, tag_size, map_ptr, std_ptr, poses_ptr, result_ptr,
                             world_id=-1, max_iters=30, stream=0, huber_px=0.0, slot_weight_ptr=0, tag_sizes=None, cov=None):
        """asl_map_rig_frames_device: obs_ptr (n_cams x n_frames x max_tags asl_obs, camera-major), rig_ptr (n_cams asl_rig_camera,
        complete when the call is made) and the outputs of build_map_device (slot_weight_ptr: n_cams x n_frames x max_tags
        doubles or 0) are device addresses; enqueued on `stream` after one wait for the problem size.  tag_sizes ({id: size} or
        n_ids sizes, on the host): asl_map_rig_sized_frames_device.  cov as in build_map_device: asl_mapcov_rig_frames_device."""
        self._map_call(True, obs_ptr, [int(n_cams), int(n_frames), int(max_tags)], n_ids, [rig_ptr], True, tag_size, tag_sizes, world_id, huber_px,
                       max_iters, (map_ptr, std_ptr, poses_ptr, result_ptr), slot_weight_ptr, stream, cov)

    def _map_host(self, o, n_frames, n_ids, dims, model, rig, tag_size, tag_sizes, world_id, huber_px, max_iters, with_std, with_slot_weight,
                  with_cov=False):
        """the host form of _map_call on the block o: the outputs allocated, build_map's items back; with_cov: one more item,
        (cov_slot (n_ids,) int32, the 6 n_cov x 6 n_cov joint covariance).  The matrix is sized by the distinct ids of the block's
        flags & 1 slots, which bounds the tags of the problem."""
        res = np.zeros((), dtype=MAP_RESULT_DTYPE)
        tmap = np.zeros(max(int(n_ids), 1), dtype=MAP_TAG_DTYPE)
        std = np.zeros((max(int(n_ids), 1), 6), dtype=np.float64) if with_std else None
        poses = np.zeros(n_frames, dtype=CAM_POSE_DTYPE)
        weight = np.zeros(o.shape, dtype=np.float64) if with_slot_weight else None
        cov = slot = mat = None
        if with_cov:
            seen = np.unique(o["id"][(o["flags"] & 1) != 0])
            cap = max(int(((seen >= 0) & (seen < int(n_ids))).sum()) - 1, 1)
            slot, mat = np.full(max(int(n_ids), 1), -1, dtype=np.int32), np.zeros((6 * cap, 6 * cap), dtype=np.float64)
            cov = (slot.ctypes.data, mat.ctypes.data, cap)
        self._map_call(False, _data(o), dims, n_ids, model, rig, tag_size, tag_sizes, world_id, huber_px, max_iters,
                       (tmap.ctypes.data, std.ctypes.data if with_std else None, _data(poses), res.ctypes.data),
                       weight.ctypes.data if with_slot_weight else None, cov=cov)
        out = (res, tmap, std, poses, weight) if with_slot_weight else (res, tmap, std, poses)
        if with_cov:
            n = 6 * int((slot >= 0).sum())
            out += ((slot, np.ascontiguousarray(mat[:n, :n])),)
        return out

    def _map_call(self, device, obs, dims, n_ids, model, rig, tag_size, tag_sizes, world_id, huber_px, max_iters, outs, weight, stream=0, cov=None):
        """The one tag-map call.  Its entry point, _batch or (device) _frames_device, whose addresses are then the device's:

            rig  tag_sizes  huber_px or weight   entry
            no   no         no                   asl_map            (no huber_px, no slot weights in its list)
            no   no         yes                  asl_map_robust
            no   yes        any                  asl_map_sized      (tag_sizes after tag_size)
            yes  no         any                  asl_map_rig
            yes  yes        any                  asl_map_rig_sized  (tag_sizes after tag_size)

        cov, (cov_slot, map_cov, cap_tags): asl_mapcov / asl_mapcov_rig, the sized lists (tag_sizes may be None there) with
        the three after the slot weights.
        dims: the block's extents; model: K, dist, n_dist or [the rig table's address]; outs: map, std (optional), poses, result."""
        sized = tag_sizes is not None
        robust = bool(rig or sized or huber_px or cov or (weight if device else weight is not None))
        table = _size_table(tag_sizes, n_ids) if sized else None
        req, opt = (_ptr, _opt_ptr) if device else (lambda p: p, lambda p: p)
        args = [self._h, req(obs)] + dims + [int(n_ids)] + ([req(model[0])] if rig else model) + [float(tag_size)]
        if sized or cov:
            args.append(table.ctypes.data_as(C.POINTER(C.c_float)) if sized else None)
        args += [int(world_id)] + ([float(huber_px)] if robust else []) + [int(max_iters), req(outs[0]), opt(outs[1]), req(outs[2]), req(outs[3])]
        if robust:
            args.append(opt(weight))
        if cov:
            args += [req(cov[0]), req(cov[1]), int(cov[2])]
        if device:
            args.append(_ptr(stream))
        name = "asl_map" + ("_rig" if rig else "") + ("_sized" if sized else "" if rig or not robust else "_robust")
        if cov:
            name = "asl_mapcov" + ("_rig" if rig else "")
        check(getattr(self._L, name + ("_frames_device" if device else "_batch"))(*args))

    def smooth(self, obs, tag_map, K, dist, tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, seed=None,
               with_cov=False, huber_px=0.0, times=None):
        """asl_smooth_batch: host records obs (n_frames, max_tags) OBS_DTYPE of one camera's consecutive frames against tag_map
        -> ((n_frames,) CAM_POSE_DTYPE, world<-camera for EVERY frame, SMOOTH_RESULT_DTYPE record): the reprojection error of
        all frames (corner sigma sigma_px) plus a random-walk motion prior between consecutive frames (sigma_rot rad,
        sigma_trans scene units per frame step).  seed: (n_frames,) CAM_POSE_DTYPE as localize() returns them for the same
        obs; None: that localisation runs first.
        with_cov: asl_smooth_cov_batch -> (poses, result, (n_frames,) POSE_COV_DTYPE), every pose's marginal covariance under
        the three sigmas (the same poses and result, byte for byte).
        huber_px > 0: asl_smooth_robust_sequences_batch with the one sequence -- a Huber loss of that many pixels on every
        corner's residual; a frame's n_rejected and the result's n_soft count the slots it down-weighted.  0.0: the calls above.
        times: (n_frames,) float64, strictly increasing, any unit -- asl_smooth_timed_sequences_batch with the one sequence:
        sigma_rot and sigma_trans are per unit of that time, a pair of frames dt apart is held by the prior / sqrt(dt).  Bad
        times (not finite, not increasing) give result status 4, no error.  None: one frame step is one unit, the calls above.
        tag_size is the size of the map entries whose size is 0, as in localize; so it is in smooth_sequences and smooth_rig."""
        o = _obs_records(obs)
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        return self._smooth_host(o, [o.shape[0], o.shape[1]], tag_map, [Kp, dpp, nd], False, tag_size, seed, times, None,
                                 (sigma_px, sigma_rot, sigma_trans), huber_px, max_iters, with_cov)

    def smooth_device(self, obs_ptr, n_frames, max_tags, map_ptr, n_ids, seed_ptr, out_ptr, result_ptr, K, dist, tag_size, sigma_px=1.0,
                      sigma_rot=0.05, sigma_trans=0.5, max_iters=20, stream=0, cov_ptr=None, huber_px=0.0, times_ptr=None):
        """asl_smooth_frames_device: obs_ptr (n_frames x max_tags asl_obs), map_ptr (n_ids asl_map_tag), seed_ptr (n_frames
        asl_cam_pose, as localize_device wrote them), out_ptr (n_frames asl_cam_pose) and result_ptr (one asl_smooth_result)
        are device addresses; enqueued on `stream`, no wait.  cov_ptr not None (n_frames asl_pose_cov):
        asl_smooth_cov_frames_device.  huber_px > 0: asl_smooth_robust_sequences_device with the one sequence.  times_ptr not
        None (n_frames doubles on the device): asl_smooth_timed_sequences_device with the one sequence."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        self._smooth_call(True, obs_ptr, [int(n_frames), int(max_tags)], map_ptr, n_ids, [Kp, dpp, nd], False, tag_size, seed_ptr, times_ptr, None,
                          (sigma_px, sigma_rot, sigma_trans), huber_px, max_iters, (out_ptr, result_ptr, cov_ptr), cov_ptr is not None, stream)

    @staticmethod
    def _seq_start(seq_start, n_frames):
        """the offsets as the C ABI takes them: (array to keep alive, pointer, n_seq).  Every refusal is the library's
        (ASL_EINVAL -> AslError); an offset that does not fit an int32 becomes -1 here, which the library refuses, so that the
        cast cannot wrap into a valid one"""
        ss = np.atleast_1d(np.asarray(seq_start, dtype=np.int64)).ravel()
        ss = np.where((ss < 0) | (ss > 0x7fffffff), -1, ss).astype(np.int32)
        if len(ss) == 0:
            ss = np.full(1, -1, dtype=np.int32)
        return ss, ss.ctypes.data_as(C.POINTER(C.c_int32)), len(ss) - 1

    def smooth_sequences(self, obs, seq_start, tag_map, K, dist, tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20,
                         seed=None, with_cov=False, huber_px=0.0, times=None):
        """asl_smooth_sequences_batch: smooth() for several sequences in one call, solved side by side.  obs (n_frames, max_tags)
        OBS_DTYPE holds the sequences end to end, sequence k the frames seq_start[k]:seq_start[k + 1] (n_seq + 1 offsets, from
        0 to n_frames) -> ((n_frames,) CAM_POSE_DTYPE, (n_seq,) SMOOTH_RESULT_DTYPE[, (n_frames,) POSE_COV_DTYPE]): for every
        sequence the bytes smooth() returns for its frames alone.  The map, the camera, the sigmas and max_iters are shared,
        and so is huber_px (> 0: asl_smooth_robust_sequences_batch, as in smooth()).  times: (n_frames,) float64, every
        sequence's own frame times end to end (asl_smooth_timed_sequences_batch, as in smooth()); they need to increase inside a
        sequence only, and a sequence with bad times has result status 4 while the others are solved."""
        o = _obs_records(obs)
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        return self._smooth_host(o, [o.shape[0], o.shape[1]], tag_map, [Kp, dpp, nd], False, tag_size, seed, times, seq_start,
                                 (sigma_px, sigma_rot, sigma_trans), huber_px, max_iters, with_cov)

    def smooth_sequences_device(self, obs_ptr, n_frames, max_tags, map_ptr, n_ids, seed_ptr, seq_start, out_ptr, results_ptr, K, dist,
                                tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, stream=0, cov_ptr=None, huber_px=0.0,
                                times_ptr=None):
        """asl_smooth_sequences_device: smooth_device for several sequences; seq_start is a HOST array of n_seq + 1 offsets,
        results_ptr n_seq asl_smooth_result on the device, cov_ptr None or n_frames asl_pose_cov.  Enqueued on `stream`, no
        wait; seq_start is read before this returns.  huber_px > 0: asl_smooth_robust_sequences_device.  times_ptr not None
        (n_frames doubles on the device): asl_smooth_timed_sequences_device."""
        keep, Kp, dpp, nd = _camera(K, dist, square=True)
        self._smooth_call(True, obs_ptr, [int(n_frames), int(max_tags)], map_ptr, n_ids, [Kp, dpp, nd], False, tag_size, seed_ptr, times_ptr, seq_start,
                          (sigma_px, sigma_rot, sigma_trans), huber_px, max_iters, (out_ptr, results_ptr, cov_ptr), cov_ptr is not None, stream)

    def smooth_rig(self, obs, tag_map, rig, tag_size, sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, seed=None, seq_start=None,
                   times=None, huber_px=0.0, with_cov=False):
        """asl_smooth_rig_sequences_batch: smooth_sequences() for a rig.  Host records obs (n_cams, n_frames, max_tags) OBS_DTYPE,
        camera-major, of the rig's consecutive frames against tag_map and the camera table rig ((n_cams,) RIG_CAMERA_DTYPE, or a
        rig.Rig) -> ((n_frames,) CAM_POSE_DTYPE, world<-rig for EVERY frame, SMOOTH_RESULT_DTYPE record[, (n_frames,)
        POSE_COV_DTYPE with with_cov]).  seed: (n_frames,) CAM_POSE_DTYPE as localize_rig() returns them for the same obs; None:
        that localisation runs first.  seq_start: None (one sequence, one result record), or n_seq + 1 offsets from 0 to
        n_frames -> (n_seq,) result records.  times, huber_px: as in smooth()."""
        o = np.ascontiguousarray(obs, dtype=OBS_DTYPE)
        if o.ndim != 3:
            raise ValueError("obs must be (n_cams, n_frames, max_tags) asl_obs records")
        r = _rig_records(rig)
        if len(r) != o.shape[0]:
            raise ValueError("the rig has %d cameras, obs has %d" % (len(r), o.shape[0]))
        return self._smooth_host(o, list(o.shape), tag_map, [_data(r)], True, tag_size, seed, times, seq_start, (sigma_px, sigma_rot, sigma_trans),
                                 huber_px, max_iters, with_cov)

    def smooth_rig_device(self, obs_ptr, n_cams, n_frames, max_tags, map_ptr, n_ids, rig_ptr, seed_ptr, out_ptr, results_ptr, tag_size,
                          sigma_px=1.0, sigma_rot=0.05, sigma_trans=0.5, max_iters=20, seq_start=None, stream=0, times_ptr=None, huber_px=0.0,
                          cov_ptr=None):
        """asl_smooth_rig_sequences_device: obs_ptr (n_cams x n_frames x max_tags asl_obs, camera-major), map_ptr (n_ids
        asl_map_tag), rig_ptr (n_cams asl_rig_camera, complete when the call is made), seed_ptr (n_frames asl_cam_pose, as
        localize_rig_device wrote them), out_ptr (n_frames asl_cam_pose) and results_ptr (n_seq asl_smooth_result) are device
        addresses; seq_start: None (the one sequence) or a HOST array of n_seq + 1 offsets; times_ptr: None or n_frames doubles
        on the device; cov_ptr: None or n_frames asl_pose_cov.  Enqueued on `stream` after the table's check."""
        self._smooth_call(True, obs_ptr, [int(n_cams), int(n_frames), int(max_tags)], map_ptr, n_ids, [rig_ptr], True, tag_size, seed_ptr, times_ptr,
                          seq_start, (sigma_px, sigma_rot, sigma_trans), huber_px, max_iters, (out_ptr, results_ptr, cov_ptr), cov_ptr is not None, stream)

    def _smooth_host(self, o, dims, tag_map, model, rig, tag_size, seed, times, seq_start, sigmas, huber_px, max_iters, with_cov):
        """the host form of _smooth_call on the block o: seed and times checked against its frames, the outputs allocated ->
        (poses, result(s)[, cov]); one result record where seq_start is None"""
        m = _map_records(tag_map)
        n = dims[-2]
        sd = None if seed is None else np.ascontiguousarray(seed, dtype=CAM_POSE_DTYPE).ravel()
        if sd is not None and len(sd) != n:
            raise ValueError("seed must hold one pose per frame")
        tm = None if times is None else np.ascontiguousarray(times, dtype=np.float64).ravel()
        if tm is not None and len(tm) != n:
            raise ValueError("times must hold one value per frame")
        out = np.zeros(n, dtype=CAM_POSE_DTYPE)
        res = np.zeros(1 if seq_start is None else max(np.size(seq_start) - 1, 0), dtype=SMOOTH_RESULT_DTYPE)
        cov = np.zeros(n, dtype=POSE_COV_DTYPE) if with_cov else None
        n_seq = self._smooth_call(False, _data(o), dims, _data(m), len(m), model, rig, tag_size, None if sd is None else sd.ctypes.data,
                                  None if tm is None else tm.ctypes.data_as(_DP), seq_start, sigmas, huber_px, max_iters,
                                  (_data(out), res.ctypes.data, _data(cov) if with_cov else None), with_cov)
        if seq_start is None:
            res = res.reshape(()) if n_seq is None else res[0]
        return (out, res, cov) if with_cov else (out, res)

    def _smooth_call(self, device, obs, dims, tag_map, n_ids, model, rig, tag_size, seed, times, seq_start, sigmas, huber_px, max_iters, outs,
                     with_cov, stream=0):
        """The one sequence-localisation call.  Its entry point, _batch or (device) _frames_device for the first two rows and
        _device for the others, whose addresses are then the device's:

            rig  times  huber_px  seq_start  cov   entry
            no   none   0         None       no    asl_smooth
            no   none   0         None       yes   asl_smooth_cov
            no   none   0         given      any   asl_smooth_sequences         (seq_start, n_seq after seed)
            no   none   != 0      any        any   asl_smooth_robust_sequences  (huber_px after the sigmas; [0, n] for None)
            no   given  any       any        any   asl_smooth_timed_sequences   (times after seed)
            yes  any    any       any        any   asl_smooth_rig_sequences     (times, which may be NULL, after seed)

        dims: the block's extents, n_frames the last but one; model: K, dist, n_dist or [the rig table's address]; outs: poses,
        result(s), cov (NULL without with_cov).  Returns n_seq as the entry got it, None for the two entries without offsets."""
        req, opt = (_ptr, _opt_ptr) if device else (lambda p: p, lambda p: p)
        timed = bool(rig or times is not None)
        robust = bool(timed or huber_px != 0.0)
        plain = not robust and seq_start is None
        ss, ssp, n_seq = self._seq_start([0, dims[-2]] if seq_start is None else seq_start, dims[-2])
        args = [self._h, req(obs)] + dims + [req(tag_map), int(n_ids)] + ([opt(model[0])] if rig else model) + [float(tag_size), req(seed)]
        args += ([opt(times)] if timed else []) + ([] if plain else [ssp, n_seq]) + [float(s) for s in sigmas]
        args += ([float(huber_px)] if robust else []) + [int(max_iters), req(outs[0]), req(outs[1])] + ([opt(outs[2])] if with_cov or not plain else [])
        if device:
            args.append(_ptr(stream))
        if plain:
            name = "asl_smooth" + ("_cov" if with_cov else "") + ("_frames_device" if device else "_batch")
        else:
            name = "asl_smooth_%ssequences" % ("rig_" if rig else "timed_" if timed else "robust_" if robust else "") + ("_device" if device else "_batch")
        check(getattr(self._L, name)(*args))
        return None if plain else n_seq

    def collect_view(self):
        """Wait for the submitted batch; (dets, poses or None, n_per_frame) as numpy VIEWS of the detector's page-locked result
        buffers (asl_collect_batch_view: no copy) -- valid until the next submit on this detector."""
        n_frames, want_poses = self._inflight
        pd, pp, pn, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        check(self._L.asl_collect_batch_view(self._h, C.byref(pd), C.byref(pp), C.byref(pn), C.byref(n)))
        nd = n.value

        def view(ptr, dtype, count):
            if not ptr or count == 0:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(ptr), dtype=dtype, count=count)
        dets = view(pd.value, DET_DTYPE, nd)
        poses = view(pp.value, POSE_DTYPE, nd) if (want_poses and pp.value) else None
        npf = view(pn.value, np.dtype(np.uint32), n_frames)
        return dets, poses, npf

    def collect(self, max_per_frame=64):
        """Wait for the submitted batch; returns (dets, poses or None, n_per_frame).  The arrays are views into
        buffers owned by the detector, valid until its next collect()."""
        n_frames, want_poses = self._inflight
        cap = n_frames * max_per_frame
        out, poses = self._result_buffers(cap, want_poses)
        npf = (C.c_int * n_frames)()
        n = C.c_int()
        check(self._L.asl_collect_batch(self._h, out.ctypes.data, poses.ctypes.data if want_poses else None, cap, npf, C.byref(n)))
        if n.value > cap:
            raise AslError("more than %d detections per frame on average; raise max_per_frame" % max_per_frame)
        return out[:n.value], (poses[:n.value] if want_poses else None), np.frombuffer(npf, dtype=np.int32)

    def _result_buffers(self, cap, want_poses):
        """The detection and pose buffers kept across calls, grown to cap records (fresh multi-MB arrays cost ~1 ms of page
        faults per call); the pose buffer is None without poses."""
        if self._outbuf is None or len(self._outbuf) < cap:
            self._outbuf = np.empty(cap, dtype=DET_DTYPE)
        if want_poses and (self._posebuf is None or len(self._posebuf) < cap):
            self._posebuf = np.empty(cap, dtype=POSE_DTYPE)
        return self._outbuf, (self._posebuf if want_poses else None)

    def solve_pnp(self, corners, K, dist, tag_size):
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 4, 2))
        N = c.shape[0]
        keep, Kp, dpp, nd = _camera(K, dist)
        rvec = np.zeros((N, 3)); tvec = np.zeros((N, 3)); T = np.zeros((N, 4, 4)); ok = np.zeros(N, np.uint8)
        check(self._L.asl_solve_pnp_batch(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), Kp, dpp, nd, float(tag_size),
                                          rvec.ctypes.data_as(_DP), tvec.ctypes.data_as(_DP), T.ctypes.data_as(_DP),
                                          ok.ctypes.data_as(C.POINTER(C.c_uint8)), N))
        return rvec, tvec, T, ok.astype(bool)

    def gn_solve(self, cam_T, tag_T, obs_cam, obs_tag, obs_corners, K, tag_size, fixed_tag=0, iters=10):
        """Pose-graph Levenberg-Marquardt on the device (asl_gn_solve).  cam_T (P,4,4) world<-camera,
        tag_T (L,4,4) world<-tag, observations (cam index, tag index, 4x2 pixel corners).
        Returns refined (cam_T, tag_T, stats=[cost0, cost, accepted])."""
        cam = np.ascontiguousarray(cam_T, dtype=np.float64).reshape(-1, 16).copy()
        tag = np.ascontiguousarray(tag_T, dtype=np.float64).reshape(-1, 16).copy()
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32)
        ot = np.ascontiguousarray(obs_tag, dtype=np.int32)
        corners = np.ascontiguousarray(obs_corners, dtype=np.float64).reshape(-1, 8)
        Kc = np.ascontiguousarray(K, dtype=np.float64)
        stats = np.zeros(3)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        check(self._L.asl_gn_solve(self._h, cam.shape[0], tag.shape[0], len(oc), oc.ctypes.data_as(ip), ot.ctypes.data_as(ip),
                                   corners.ctypes.data_as(dp), Kc.ctypes.data_as(dp), float(tag_size), int(fixed_tag),
                                   cam.ctypes.data_as(dp), tag.ctypes.data_as(dp), int(iters), stats.ctypes.data_as(dp)))
        return cam.reshape(-1, 4, 4), tag.reshape(-1, 4, 4), stats

    # -- introspection for the parity tests ------------------------------------------------
    def debug_counters(self):
        buf = np.zeros(18, dtype=np.int64)
        n = C.c_size_t()
        check(self._L.asl_debug_fetch(self._h, 5, buf.ctypes.data, buf.nbytes, C.byref(n)))
        return buf

    def debug_image(self, what):
        c = self.debug_counters()
        B, sw, sh = int(c[0]), int(c[1]), int(c[2])
        dt = np.uint8 if what in (0, 1, 9) else np.uint32
        buf = np.zeros((B, sh, sw), dtype=dt)
        n = C.c_size_t()
        check(self._L.asl_debug_fetch(self._h, what, buf.ctypes.data, buf.nbytes, C.byref(n)))
        return buf

    def debug_quads(self, cap=65536):
        buf = np.zeros(cap, dtype=QUAD_DTYPE)
        n = C.c_size_t()
        check(self._L.asl_debug_fetch(self._h, 4, buf.ctypes.data, buf.nbytes, C.byref(n)))
        return buf[:n.value]

    def debug_clusters(self):
        """(n, 3) uint64: key, point count, hash of the sorted point records of every cluster of the last batch, by key."""
        ncl = int(self.debug_counters()[3])
        buf = np.zeros((max(ncl, 1), 3), dtype=np.uint64)
        n = C.c_size_t()
        check(self._L.asl_debug_fetch(self._h, 6, buf.ctypes.data, buf.nbytes, C.byref(n)))
        return buf[:n.value]

    def debug_refit(self, reps):
        """Re-run the quad fit of the last batch `reps` times; int64[7]: reps, quads differing from the first run, by size class."""
        buf = np.zeros(7, dtype=np.int64)
        check(self._L.asl_debug_refit(self._h, int(reps), buf.ctypes.data, len(buf)))
        return buf

    def debug_dedup(self, dets, keys, n_frames, cap_per_frame=1024):
        """asl_debug_dedup: the de-duplication stage alone on DET_DTYPE records and their uint64 cluster keys (low 48 bits) ->
        (survivors in device order, (n_frames,) int32 counts, int64[3]: survivors, records past a full list, frames above 1024)."""
        d = np.ascontiguousarray(dets, dtype=DET_DTYPE).ravel()
        k = np.ascontiguousarray(keys, dtype=np.uint64).ravel()
        if len(k) != len(d):
            raise ValueError("one key per record")
        out = np.zeros(max(len(d), 1), dtype=DET_DTYPE)
        npf = np.zeros(max(int(n_frames), 1), dtype=np.int32)
        cnt = np.zeros(3, dtype=np.int64)
        check(self._L.asl_debug_dedup(self._h, d.ctypes.data, k.ctypes.data, len(d), int(n_frames), int(cap_per_frame), out.ctypes.data,
                                      len(out), npf.ctypes.data, cnt.ctypes.data, len(cnt)))
        return out[:int(cnt[0])], npf, cnt

    def debug_gn_cholesky(self, A, b):
        """asl_debug_gn_cholesky: the back-end's blocked Cholesky, back substitution and diag(A^-1) on a dense symmetric A
        (n x n, n = 6 x tags) and right-hand side b -> dict(L, y, x, Linv (blocks, 48, 48), var, fail)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = A.shape[0]
        if A.shape != (n, n) or b.shape != (n,):
            raise ValueError("A must be square and b of its size")
        nblk = (n + 47) // 48
        L, y, x, var, Linv = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((max(nblk, 1), 48, 48))
        flag = C.c_int32(-1)
        ptr = lambda a: a.ctypes.data_as(_DP)
        check(self._L.asl_debug_gn_cholesky(self._h, ptr(A), ptr(b), n, ptr(L), L.size, ptr(y), ptr(x), ptr(var), n, ptr(Linv), Linv.size,
                                            C.byref(flag)))
        return dict(L=L, y=y, x=x, Linv=Linv, var=var, fail=int(flag.value))

    def debug_gn_step(self, cam_T, tag_T, obs_cam, obs_tag, obs_corners, K, tag_size, fixed_tag, lam, want=GN_STEP_ITEMS):
        """asl_debug_gn_step: one damped step of gn_solve's problem at damping lam, stage by stage -> dict of the items in
        `want` (GN_STEP_ITEMS; shapes: gn_step_shapes) and `fail`.  The poses are not changed."""
        cam = np.ascontiguousarray(cam_T, dtype=np.float64).reshape(-1, 16)
        tag = np.ascontiguousarray(tag_T, dtype=np.float64).reshape(-1, 16)
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32)
        ot = np.ascontiguousarray(obs_tag, dtype=np.int32)
        corners = np.ascontiguousarray(obs_corners, dtype=np.float64).reshape(-1, 8)
        Kc = np.ascontiguousarray(K, dtype=np.float64)
        shapes = gn_step_shapes(cam.shape[0], tag.shape[0], len(oc))
        res = {k: np.zeros(shapes[k]) for k in want}
        spans = (DebugSpan * len(GN_STEP_ITEMS))()
        for i, k in enumerate(GN_STEP_ITEMS):
            if k in res:
                spans[i].p, spans[i].n = res[k].ctypes.data_as(_DP), res[k].size
        flag = C.c_int32(-1)
        ip = C.POINTER(C.c_int32)
        check(self._L.asl_debug_gn_step(self._h, cam.shape[0], tag.shape[0], len(oc), oc.ctypes.data_as(ip), ot.ctypes.data_as(ip),
                                        corners.ctypes.data_as(_DP), Kc.ctypes.data_as(_DP), float(tag_size), int(fixed_tag),
                                        cam.ctypes.data_as(_DP), tag.ctypes.data_as(_DP), float(lam), spans, len(spans), C.byref(flag)))
        res["fail"] = int(flag.value)
        return res

    def debug_division_check(self, exponent_limit=100):
        """(pairs, mismatches) of div_by(a, recip_of(d)) against a / d on the device, exponents within +-exponent_limit."""
        buf = np.zeros(2, dtype=np.int64)
        check(self._L.asl_debug_division_check(self._h, int(exponent_limit), buf.ctypes.data, len(buf)))
        return int(buf[0]), int(buf[1])

    def phase_cycles(self, reset=True):
        buf = (C.c_uint64 * 64)()
        check(self._L.asl_debug_phase_cycles(self._h, buf, len(buf), 1 if reset else 0))
        return np.array(list(buf), dtype=np.uint64)

    def set_profiling(self, on=True):
        check(self._L.asl_set_profiling(self._h, 1 if on else 0))

    def stage_times(self):
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        n = C.c_int()
        check(self._L.asl_stage_times(self._h, names, ms, 32, C.byref(n)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}
