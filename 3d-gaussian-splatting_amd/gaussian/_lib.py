"""ctypes loader for libgs_amd.so (the C ABI in include/gs_abi.h).

There is NO CPU fallback: if the shared library is missing or cannot be loaded, importing
``gaussian`` raises.  The library is built in-tree by ``gs_build.build()`` /
``__graft_entry__.build()``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GS_AMD_LIB: an experiment variant of the library (gs_build.build(outdir=...), tools/ab_variants.py); the product
# always loads the in-tree build
LIB_PATH = os.environ.get("GS_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "libgs_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"libgs_amd.so not found at {LIB_PATH}: build it with `python __graft_entry__.py` "
        "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the rasterizer.")

lib = C.CDLL(LIB_PATH)

vp, i64, i32, f32, ci, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int, C.c_size_t


class GsFrame(C.Structure):
    """Mirror of ``struct gs_frame`` (include/gs_abi.h)."""

    _fields_ = [
        ("N", i64), ("color_dim", i32), ("scale_activation", i32),
        ("pos", vp), ("quat", vp), ("scale", vp), ("opa", vp), ("rgb", vp),
        ("rot", f32 * 9), ("tran", f32 * 3),
        ("near_plane", f32), ("half_width", f32), ("half_height", f32),
        ("width", i32), ("height", i32),
        ("focal_x", f32), ("focal_y", f32),
        ("tile_length_x", f32), ("tile_length_y", f32), ("leftmost", f32), ("topmost", f32),
        ("thresh", f32),
        ("rays_o", f32 * 3), ("lefttop", f32 * 3), ("vec_dx", f32 * 3), ("vec_dy", f32 * 3),
        ("max_pairs", i64), ("workspace", vp), ("workspace_bytes", sz),
        ("image", vp), ("image_padded", vp),
        ("training", i32), ("sort_mode", i32), ("tile_culling_method", i32),
        ("async_", vp), ("flags", i32),  # ABI 3 (`async` is a Python keyword)
        # GS_FRAME_AUX (read by the library only when the flag is set)
        ("depth", vp), ("alpha", vp), ("aux_padded", vp), ("aux_workspace", vp), ("aux_workspace_bytes", sz),
        ("grad_depth", vp), ("grad_alpha", vp),
        # GS_FRAME_POSE_GRAD (read by the library only when the flag is set)
        ("grad_rot", vp), ("grad_tran", vp), ("pose_workspace", vp), ("pose_workspace_bytes", sz),
    ]


class GsFrameScene(GsFrame):
    """Mirror of ``struct gs_frame_scene``: a ``gs_frame`` followed by the GS_FRAME_SCENE_PACK fields (read by the library
    only when the flag is set).  An instance is accepted wherever a ``GsFrame`` is (same address, the fields behind it)."""

    _fields_ = [("scene_pack_a", vp), ("scene_pack_b", vp), ("scene_pack_a_bytes", sz), ("scene_pack_b_bytes", sz)]


class GsFramePP(GsFrameScene):
    """Mirror of ``struct gs_frame_pp``: a ``gs_frame_scene`` followed by the GS_FRAME_PRINCIPAL_POINT fields (read by the
    library only when the flag is set).  An instance is accepted wherever a ``GsFrame`` is."""

    _fields_ = [("pp_dx", C.c_double), ("pp_dy", C.c_double)]


class GsFrameDP(GsFramePP):
    """Mirror of ``struct gs_frame_dp``: a ``gs_frame_pp`` followed by the GS_FRAME_DEVICE_POSE field (read by the library only
    when the flag is set).  An instance is accepted wherever a ``GsFrame`` is."""

    _fields_ = [("pose_dev", vp)]


GS_FRAME_EMIT_SORTED_KEYS = 1
GS_FRAME_SLICE_SORT = 2
GS_FRAME_TABLE_BIN = 4
GS_FRAME_SERIAL_LONG_LISTS = 8
GS_FRAME_LONG_LISTS = 16
GS_FRAME_STRIP_BIN = 32
GS_FRAME_BWD_ROWS = 64
GS_FRAME_LONG_SORT = 128
GS_FRAME_OCCLUSION_CULL = 256
GS_FRAME_CULL_DILATE = 512
GS_FRAME_CULL_DILATE_NEAR = 1024
GS_FRAME_AUX = 2048
GS_FRAME_POSE_GRAD = 4096
GS_FRAME_SCENE_PACK = 8192
GS_FRAME_PRINCIPAL_POINT = 16384
GS_FRAME_DEVICE_POSE = 32768
GS_FRAME_CULL_REPEAT = 65536


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


gs_last_error = _sig("gs_last_error", C.c_char_p)
gs_abi_version = _sig("gs_abi_version", ci)
gs_culling = _sig("gs_culling", ci)
gs_world2camera = _sig("gs_world2camera", ci, vp, vp, vp, vp, i64, vp)
gs_world2camera_backward = _sig("gs_world2camera_backward", ci, vp, vp, vp, i64, vp)
gs_jacobian = _sig("gs_jacobian", ci, vp, vp, i64, vp)
gs_global_culling = _sig("gs_global_culling", ci, vp, vp, vp, vp, vp, i64, f32, f32, f32, vp, vp, vp, vp)
gs_global_culling_backward = _sig("gs_global_culling_backward", ci, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp,
                                  vp, vp)
gs_calc_tile_list = _sig("gs_calc_tile_list", ci, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, f32, ci, f32, f32,
                         i32, i32, f32, f32, vp)
gs_gather_gaussians = _sig("gs_gather_gaussians", ci, vp, vp, vp, vp, i64, i64, i64, vp)
gs_draw = _sig("gs_draw", ci, vp, vp, vp, vp, vp, vp, i32, i32, i64, f32, f32, ci, ci, ci, vp, vp, vp, vp, ci, vp)
gs_draw_backward_workspace_bytes = _sig("gs_draw_backward_workspace_bytes", sz, i64, i32, i32)
gs_draw_backward = _sig("gs_draw_backward", ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, f32, f32,
                        ci, ci, ci, vp, vp, vp, vp, ci, vp, sz, vp)
gs_sort_pairs_tmp_bytes = _sig("gs_sort_pairs_tmp_bytes", sz, i64)
gs_sort_pairs = _sig("gs_sort_pairs", ci, vp, vp, vp, vp, vp, i64, ci, vp, sz, C.POINTER(ci), vp)
gs_sort_pairs_bits = _sig("gs_sort_pairs_bits", ci, vp, vp, vp, vp, vp, i64, ci, ci, vp, sz, C.POINTER(ci), vp)
gs_frame_workspace_bytes = _sig("gs_frame_workspace_bytes", sz, i64, i64, i32, i32, i32, i32)
gs_frame_aux_workspace_bytes = _sig("gs_frame_aux_workspace_bytes", sz, i64, i32, i32, i32)
gs_frame_pose_workspace_bytes = _sig("gs_frame_pose_workspace_bytes", sz, i64)
gs_scene_pack_bytes = _sig("gs_scene_pack_bytes", sz, i64, C.POINTER(sz), C.POINTER(sz))
gs_scene_pack_build = _sig("gs_scene_pack_build", ci, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp)
gs_frame_reads_scene_pack = _sig("gs_frame_reads_scene_pack", ci, C.POINTER(GsFrame))
gs_frame_forward = _sig("gs_frame_forward", ci, C.POINTER(GsFrame), vp)
gs_frame_backward = _sig("gs_frame_backward", ci, C.POINTER(GsFrame), vp, vp, vp, vp, vp, vp, vp)
gs_frame_backward_part = _sig("gs_frame_backward_part", ci, C.POINTER(GsFrame), vp, vp, vp, vp, vp, vp, i32, vp)
GS_BWD_RASTER, GS_BWD_GEOMETRY, GS_BWD_COLOR = 1, 2, 4
gs_frame_backward_slice = _sig("gs_frame_backward_slice", ci, C.POINTER(GsFrame), vp, vp, vp, vp, vp, i32, i64, i64, vp)
gs_frame_project_slices = _sig("gs_frame_project_slices", ci, C.POINTER(GsFrame), C.POINTER(i32), C.POINTER(i64))
gs_frame_forward_project = _sig("gs_frame_forward_project", ci, C.POINTER(GsFrame), i32, i32, vp)
gs_frame_forward_rest = _sig("gs_frame_forward_rest", ci, C.POINTER(GsFrame), vp)
gs_frame_forward_profile = _sig("gs_frame_forward_profile", ci, C.POINTER(GsFrame), C.POINTER(f32), vp)
gs_frame_backward_profile = _sig("gs_frame_backward_profile", ci, C.POINTER(GsFrame), vp, vp, vp, vp, vp, vp,
                                 C.POINTER(f32), vp)
gs_frame_stats_async = _sig("gs_frame_stats_async", ci, C.POINTER(GsFrame), vp, vp)
gs_frame_longest_list_async = _sig("gs_frame_longest_list_async", ci, C.POINTER(GsFrame), vp, vp)
gs_frame_stats_tagged_async = _sig("gs_frame_stats_tagged_async", ci, C.POINTER(GsFrame), C.c_uint32, vp, vp)
gs_frame_cull_fallback_async = _sig("gs_frame_cull_fallback_async", ci, C.POINTER(GsFrame), vp, vp)
gs_frame_is_occlusion_culled = _sig("gs_frame_is_occlusion_culled", ci, C.POINTER(GsFrame), C.POINTER(C.c_int32))
gs_frame_cull_second_pass = _sig("gs_frame_cull_second_pass", ci, C.POINTER(GsFrame), C.POINTER(C.c_int32))
gs_frame_debug_cut_table = _sig("gs_frame_debug_cut_table", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(C.c_int32))
gs_frame_debug_tile_compact = _sig("gs_frame_debug_tile_compact", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(C.c_int32))
gs_frame_debug_tile_cost = _sig("gs_frame_debug_tile_cost", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(C.c_int32))
GS_STATS_TAGGED_N = 15
gs_frame_debug_views = _sig("gs_frame_debug_views", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(vp),
                            C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp))

gs_frame_binning_variant = _sig("gs_frame_binning_variant", ci, C.POINTER(GsFrame))
gs_frame_debug_rects = _sig("gs_frame_debug_rects", ci, C.POINTER(GsFrame), C.POINTER(vp))
gs_frame_debug_cull_stage = _sig("gs_frame_debug_cull_stage", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                 C.POINTER(i32), C.POINTER(i64))
class GsAdamFused(C.Structure):
    """Mirror of ``struct gs_adam_fused`` (include/gs_abi.h): moments / learning rates in the order pos, quat, scale, opa, rgb."""

    _fields_ = [("exp_avg", vp * 5), ("exp_avg_sq", vp * 5), ("lr", C.c_float * 5),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("step", i64),
                ("grad_stat", vp), ("stat_mode", i32), ("skip_if_nonzero", vp)]


gs_frame_backward_adam = _sig("gs_frame_backward_adam", ci, C.POINTER(GsFrame), vp, C.POINTER(GsAdamFused), vp)
gs_frame_backward_adam_aux = _sig("gs_frame_backward_adam_aux", ci, C.POINTER(GsFrame), vp, C.POINTER(GsAdamFused), vp)
gs_frame_backward_adam_pose = _sig("gs_frame_backward_adam_pose", ci, C.POINTER(GsFrame), vp, C.POINTER(GsAdamFused), vp)
gs_frame_backward_pose = _sig("gs_frame_backward_pose", ci, C.POINTER(GsFrame), vp, i32, vp)
gs_frame_debug_tile_nproc = _sig("gs_frame_debug_tile_nproc", ci, C.POINTER(GsFrame), C.POINTER(vp))
gs_frame_debug_bwd_exec_rows = _sig("gs_frame_debug_bwd_exec_rows", ci, C.POINTER(GsFrame), C.POINTER(vp), C.POINTER(C.c_int32))

gs_adam_step = _sig("gs_adam_step", ci, vp, vp, vp, vp, i64, i32, C.POINTER(i64), C.POINTER(f32), f32, f32, f32, i64,
                    vp, i64, i64, i32, vp)
gs_adam_step_range = _sig("gs_adam_step_range", ci, vp, vp, vp, vp, i64, i64, i64, i32, C.POINTER(i64), C.POINTER(f32),
                          f32, f32, f32, i64, vp, i64, i64, i32, vp)
gs_adam_step_sharded = _sig("gs_adam_step_sharded", ci, vp, vp, vp, vp, i64, i64, i64, i64, i32, C.POINTER(i64),
                            C.POINTER(f32), f32, f32, f32, i64, vp, i64, i64, i32, vp, vp)
gs_adam_step_multi = _sig("gs_adam_step_multi", ci, vp, vp, vp, vp, i64, i32, C.POINTER(i64), C.POINTER(i64),
                          C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(f32), f32, f32, f32, i64, vp, i64, i64, i32, vp,
                          f32, vp)
gs_frame_overflow_flag = _sig("gs_frame_overflow_flag", ci, C.POINTER(GsFrame), C.POINTER(vp))
gs_grad_stat_update = _sig("gs_grad_stat_update", ci, vp, vp, i64, i32, vp)
gs_frame_async_create = _sig("gs_frame_async_create", ci, C.POINTER(vp))
gs_frame_async_wait = _sig("gs_frame_async_wait", ci, vp, vp)
gs_frame_async_destroy = _sig("gs_frame_async_destroy", ci, vp)
gs_loss_workspace_bytes = _sig("gs_loss_workspace_bytes", sz, i32, i32)
gs_loss_l1_ssim = _sig("gs_loss_l1_ssim", ci, vp, vp, i32, i32, f32, vp, vp, vp, sz, vp)
gs_loss_depth_workspace_bytes = _sig("gs_loss_depth_workspace_bytes", sz, i32, i32)
gs_loss_depth = _sig("gs_loss_depth", ci, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp, sz, vp)
gs_loss_track_workspace_bytes = _sig("gs_loss_track_workspace_bytes", sz, i32, i32)
gs_loss_track = _sig("gs_loss_track", ci, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, vp, vp, sz, vp)
gs_loss_track_gated_workspace_bytes = _sig("gs_loss_track_gated_workspace_bytes", sz, i32, i32)
gs_loss_track_gated = _sig("gs_loss_track_gated", ci, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, f32, f32, f32, f32, i32, f32,
                           vp, vp, vp, vp, vp, vp, vp, sz, vp)
gs_track_gate_mask_workspace_bytes = _sig("gs_track_gate_mask_workspace_bytes", sz, i32, i32)
gs_track_gate_mask = _sig("gs_track_gate_mask", ci, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, f32, f32, i32, vp, vp, vp, vp,
                          vp, vp, sz, vp)
gs_loss_l1_ssim_weighted = _sig("gs_loss_l1_ssim_weighted", ci, vp, vp, vp, i32, i32, f32, C.c_double, C.c_double, vp, vp, vp,
                                sz, vp)


class GsDensifyOpts(C.Structure):
    """Mirror of ``struct gs_densify_opts``."""

    _fields_ = [("taus", f32), ("delete_thresh", f32), ("grad_thresh", f32), ("clone_dt", f32),
                ("scale_activation", i32), ("grad_aggregation", i32), ("use_clone", i32), ("use_split", i32),
                ("color_dim", i32)]


gs_densify_workspace_bytes = _sig("gs_densify_workspace_bytes", sz, i64)
gs_densify_classify = _sig("gs_densify_classify", ci, vp, vp, vp, i64, C.POINTER(GsDensifyOpts), vp, vp, sz, vp)
gs_densify_apply = _sig("gs_densify_apply", ci, vp, vp, vp, vp, vp, vp, i64, C.POINTER(GsDensifyOpts), vp, vp, i64,
                        vp, vp, vp, vp, vp, i64, vp, vp, sz, vp)


class GsSeedOpts(C.Structure):
    """Mirror of ``struct gs_seed_opts``."""

    _fields_ = [("stride", i32), ("alpha_thresh", f32), ("front_rel", f32), ("scale_factor", f32), ("opa_init", f32),
                ("scale_activation", i32), ("color_dim", i32)]


class GsSeedCamera(C.Structure):
    """Mirror of ``struct gs_seed_camera``."""

    _fields_ = [("rot", f32 * 9), ("tran", f32 * 3), ("focal_x", f32), ("focal_y", f32), ("width", i32), ("height", i32)]


class GsSeedCameraPP(C.Structure):
    """Mirror of ``struct gs_seed_camera_pp``: a ``gs_seed_camera`` and the principal point's offset in pixels."""

    _fields_ = [("cam", GsSeedCamera), ("pp_dx", f32), ("pp_dy", f32)]


gs_seed_workspace_bytes = _sig("gs_seed_workspace_bytes", sz, i32, i32)
gs_seed_classify = _sig("gs_seed_classify", ci, vp, vp, vp, i32, i32, C.POINTER(GsSeedOpts), vp, vp, sz, vp)
gs_seed_apply = _sig("gs_seed_apply", ci, vp, vp, C.POINTER(GsSeedCamera), C.POINTER(GsSeedOpts), vp, vp, vp, vp, vp, i64,
                     i64, vp, vp, sz, vp)
gs_seed_apply_pp = _sig("gs_seed_apply_pp", ci, vp, vp, C.POINTER(GsSeedCameraPP), C.POINTER(GsSeedOpts), vp, vp, vp, vp, vp,
                        i64, i64, vp, vp, sz, vp)

GS_OVERLAP_MAX_VIEWS = 256


class GsOverlapOpts(C.Structure):
    """Mirror of ``struct gs_overlap_opts``."""

    _fields_ = [("stride", i32), ("near", f32), ("border", i32)]


gs_view_overlap_workspace_bytes = _sig("gs_view_overlap_workspace_bytes", sz, i32, i32, i32, i32)
gs_view_overlap_check_view = _sig("gs_view_overlap_check_view", ci, C.POINTER(GsSeedCamera), i32)
gs_view_overlap = _sig("gs_view_overlap", ci, vp, C.POINTER(GsSeedCamera), vp, i32, C.POINTER(GsOverlapOpts), vp, vp, sz, vp)
gs_view_overlap_pp = _sig("gs_view_overlap_pp", ci, vp, C.POINTER(GsSeedCameraPP), vp, vp, i32, C.POINTER(GsOverlapOpts), vp,
                          vp, sz, vp)

GS_REDUNDANCY_BINS = 8
gs_view_redundancy_workspace_bytes = _sig("gs_view_redundancy_workspace_bytes", sz, i32, i32, i32)
gs_view_redundancy = _sig("gs_view_redundancy", ci, vp, C.POINTER(GsSeedCamera), vp, i32, i32, C.POINTER(GsOverlapOpts), vp, vp,
                          sz, vp)
gs_view_redundancy_pp = _sig("gs_view_redundancy_pp", ci, vp, C.POINTER(GsSeedCameraPP), vp, vp, i32, i32,
                             C.POINTER(GsOverlapOpts), vp, vp, sz, vp)

GS_PRUNE_MAX_ARRAYS = 16


class GsPruneOpts(C.Structure):
    """Mirror of ``struct gs_prune_opts``."""

    _fields_ = [("opa_logit_min", f32), ("scale_max", f32), ("scale_activation", i32)]


class GsPruneArrays(C.Structure):
    """Mirror of ``struct gs_prune_arrays``."""

    _fields_ = [("n", i32), ("width", i32 * GS_PRUNE_MAX_ARRAYS), ("src", vp * GS_PRUNE_MAX_ARRAYS),
                ("dst", vp * GS_PRUNE_MAX_ARRAYS)]


gs_prune_workspace_bytes = _sig("gs_prune_workspace_bytes", sz, i64)
gs_prune_classify = _sig("gs_prune_classify", ci, vp, vp, i64, C.POINTER(GsPruneOpts), vp, vp, sz, vp)
gs_prune_apply = _sig("gs_prune_apply", ci, C.POINTER(GsPruneArrays), i64, i64, i64, vp, vp, sz, vp)
# (beside gs_prune_apply, as in the header: it takes gs_prune_arrays)
gs_densify_apply_state = _sig("gs_densify_apply_state", ci, C.POINTER(GsPruneArrays), i64, i64, vp, vp, sz, vp)


class GsContribOpts(C.Structure):
    """Mirror of ``struct gs_contrib_opts``."""

    _fields_ = [("w_min", f32), ("accumulate", i32)]


class GsPruneContribOpts(C.Structure):
    """Mirror of ``struct gs_prune_contrib_opts``."""

    _fields_ = [("weight_max_min", f32), ("pixels_min", C.c_uint32), ("views_min", C.c_uint32)]


gs_frame_contrib_workspace_bytes = _sig("gs_frame_contrib_workspace_bytes", sz, i64)
gs_frame_contrib = _sig("gs_frame_contrib", ci, C.POINTER(GsFrame), C.POINTER(GsContribOpts), vp, vp, sz, vp)
gs_prune_classify_contrib = _sig("gs_prune_classify_contrib", ci, vp, vp, vp, i64, C.POINTER(GsPruneOpts),
                                 C.POINTER(GsPruneContribOpts), vp, vp, sz, vp)

GS_PYRAMID_MAX_LEVELS = 4


class GsPyramidOpts(C.Structure):
    """Mirror of ``struct gs_pyramid_opts``."""

    _fields_ = [("min_valid", i32), ("edge_rel", f32)]


gs_pyramid_down = _sig("gs_pyramid_down", ci, vp, vp, i32, i32, C.POINTER(GsPyramidOpts), vp, vp, vp)

GS_ICP_LOG_DOUBLES = 40
GS_ICP_OK, GS_ICP_TOO_FEW, GS_ICP_NOT_POSITIVE = 0, 1, 2


class GsIcpModelOpts(C.Structure):
    """Mirror of ``struct gs_icp_model_opts``."""

    _fields_ = [("alpha_min", f32), ("edge_rel", f32), ("normal_step", i32)]


class GsIcpOpts(C.Structure):
    """Mirror of ``struct gs_icp_opts``."""

    _fields_ = [("stride", i32), ("dist_max", f32), ("cos_min", f32), ("min_count", i32), ("damping", C.c_double)]


class GsIcpState(C.Structure):
    """Mirror of ``struct gs_icp_state`` (it lives in device memory)."""

    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("iteration", i32), ("reserved", i32)]


gs_icp_model_bytes = _sig("gs_icp_model_bytes", sz, i32, i32)
gs_icp_workspace_bytes = _sig("gs_icp_workspace_bytes", sz, i32, i32, i32)
gs_icp_log_bytes = _sig("gs_icp_log_bytes", sz, i32)
gs_icp_model_maps = _sig("gs_icp_model_maps", ci, vp, vp, C.POINTER(GsSeedCameraPP), C.POINTER(GsIcpModelOpts), vp, vp, vp)
gs_icp_reset = _sig("gs_icp_reset", ci, vp, vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp)
gs_icp_step = _sig("gs_icp_step", ci, vp, C.POINTER(GsSeedCameraPP), vp, vp, C.POINTER(GsSeedCameraPP), C.POINTER(GsIcpOpts),
                   vp, vp, i32, i32, vp, sz, vp)

GS_POSE_LOG_HEAD = 24


class GsPoseState(C.Structure):
    """Mirror of ``struct gs_pose_state`` (it lives in device memory)."""

    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("m", C.c_double * 6), ("v", C.c_double * 6),
                ("best_R", C.c_double * 9), ("best_t", C.c_double * 3), ("best_loss", C.c_double),
                ("steps", i32), ("best_row", i32), ("skipped", i32), ("bad", i32)]


class GsPoseStepOpts(C.Structure):
    """Mirror of ``struct gs_pose_step_opts``."""

    _fields_ = [("lr_rot", C.c_double), ("lr_tran", C.c_double), ("lr_scale", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("track_best", i32), ("n_values", i32)]


gs_pose_log_bytes = _sig("gs_pose_log_bytes", sz, i32, i32)
gs_pose_reset = _sig("gs_pose_reset", ci, vp, vp, vp, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp)
gs_pose_step = _sig("gs_pose_step", ci, vp, vp, vp, vp, C.POINTER(GsPoseStepOpts), vp, vp, vp, i32, i32, vp)


class GsExposureState(C.Structure):
    """Mirror of ``struct gs_exposure_state`` (it lives in device memory)."""

    _fields_ = [("m", C.c_double * 6), ("v", C.c_double * 6), ("steps", C.c_double)]


class GsExposureAdam(C.Structure):
    """Mirror of ``struct gs_exposure_adam``."""

    _fields_ = [("state", vp), ("lr_gain", C.c_double), ("lr_bias", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("lr_scale", C.c_double), ("skip_if_nonzero", vp)]


gs_exposure_workspace_bytes = _sig("gs_exposure_workspace_bytes", sz, i32, i32)
gs_exposure_apply = _sig("gs_exposure_apply", ci, vp, vp, i32, i32, vp, vp)
gs_exposure_backward = _sig("gs_exposure_backward", ci, vp, vp, vp, i32, i32, vp, C.POINTER(GsExposureAdam), vp, sz, vp)

# Every symbol include/gs_abi.h declares (checked by tests/test_abi.py without a GPU).
EXPORTS = [
    "gs_last_error", "gs_abi_version", "gs_culling", "gs_world2camera", "gs_world2camera_backward",
    "gs_jacobian", "gs_global_culling", "gs_global_culling_backward", "gs_calc_tile_list",
    "gs_gather_gaussians", "gs_draw", "gs_draw_backward_workspace_bytes", "gs_draw_backward",
    "gs_sort_pairs_tmp_bytes", "gs_sort_pairs", "gs_sort_pairs_bits", "gs_frame_workspace_bytes",
    "gs_frame_aux_workspace_bytes", "gs_frame_pose_workspace_bytes", "gs_frame_forward",
    "gs_frame_stats_async", "gs_frame_longest_list_async", "gs_frame_stats_tagged_async", "gs_frame_cull_fallback_async", "gs_frame_is_occlusion_culled", "gs_frame_cull_second_pass", "gs_frame_debug_cut_table", "gs_frame_debug_tile_compact", "gs_frame_debug_tile_cost", "gs_frame_debug_views", "gs_frame_debug_rects", "gs_frame_debug_cull_stage", "gs_frame_binning_variant", "gs_frame_debug_tile_nproc", "gs_frame_debug_bwd_exec_rows", "gs_frame_backward", "gs_frame_backward_adam", "gs_frame_forward_profile",
    "gs_frame_backward_part", "gs_frame_async_create", "gs_frame_async_wait", "gs_frame_async_destroy",
    "gs_frame_backward_slice", "gs_frame_project_slices", "gs_frame_forward_project", "gs_frame_forward_rest",
    "gs_adam_step_multi",
    "gs_frame_backward_profile", "gs_adam_step", "gs_adam_step_range", "gs_adam_step_sharded", "gs_frame_overflow_flag", "gs_grad_stat_update", "gs_loss_workspace_bytes", "gs_loss_l1_ssim",
    "gs_loss_depth_workspace_bytes", "gs_loss_depth", "gs_frame_backward_adam_aux", "gs_frame_backward_adam_pose",
    "gs_frame_backward_pose",
    "gs_densify_workspace_bytes", "gs_densify_classify", "gs_densify_apply", "gs_densify_apply_state",
    "gs_seed_workspace_bytes", "gs_seed_classify", "gs_seed_apply",
    "gs_loss_track_workspace_bytes", "gs_loss_track",
    "gs_loss_track_gated_workspace_bytes", "gs_loss_track_gated",
    "gs_track_gate_mask_workspace_bytes", "gs_track_gate_mask", "gs_loss_l1_ssim_weighted",
    "gs_view_overlap_workspace_bytes", "gs_view_overlap_check_view", "gs_view_overlap",
    "gs_scene_pack_bytes", "gs_scene_pack_build", "gs_frame_reads_scene_pack",
    "gs_prune_workspace_bytes", "gs_prune_classify", "gs_prune_apply",
    "gs_seed_apply_pp", "gs_view_overlap_pp",
    "gs_frame_contrib_workspace_bytes", "gs_frame_contrib", "gs_prune_classify_contrib",
    "gs_pyramid_down",
    "gs_icp_model_bytes", "gs_icp_workspace_bytes", "gs_icp_log_bytes", "gs_icp_model_maps", "gs_icp_reset", "gs_icp_step",
    "gs_view_redundancy_workspace_bytes", "gs_view_redundancy", "gs_view_redundancy_pp",
    "gs_pose_log_bytes", "gs_pose_reset", "gs_pose_step",
    "gs_exposure_workspace_bytes", "gs_exposure_apply", "gs_exposure_backward",
]


def check(rc: int, what: str):
    """Map the C return convention onto the reference's: a Python RuntimeError."""
    if rc != 0:
        msg = gs_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def call(name: str, *args):
    """``check`` of the int-returning symbol ``name``, looked up when called: the error names what was called."""
    check(globals()[name](*args), name)
