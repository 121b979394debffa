/*
 * gs_abi.h -- C ABI of libgs_amd.so, the MI355X (gfx950) rasterizer library.
 *
 * This is the drop-in boundary for the hot path of WangFeng18/3d-gaussian-splatting: the
 * entry points in section A are exactly what the reference's pybind11 module `gaussian`
 * (src/bindings.cpp:21-50) binds, with torch::Tensor arguments replaced by raw device
 * pointers + explicit sizes and an explicit HIP stream.  Section B is the fused,
 * MI355X-native frame path (cull+project -> binning by tile -> per-tile depth sort ->
 * raster fwd/bwd -> project bwd) that the reference spreads over 4 native launches and ~25
 * torch kernels per frame (splatter.py:513-641).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - all arrays are contiguous, row-major, fp32 unless stated;
 *   - the caller owns every buffer; the library never allocates device memory and keeps no
 *     pointer past the call; it is re-entrant across host threads (forward is called from
 *     the main thread, backward from PyTorch's autograd thread);
 *   - every function returns 0 on success, a negative GS_E_* validation code, or a positive
 *     hipError_t; gs_last_error() returns a thread-local message for the last failure;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is
 *     what the reference launches on).
 */
#ifndef GS_ABI_H
#define GS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden; only this header's symbols are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_exposure_apply,
 *   gs_exposure_backward and gs_exposure_workspace_bytes with gs_exposure_state / gs_exposure_adam (a view's affine exposure,
 *   gain[3] and bias[3] in device memory, around any colour loss: the compensated image in front of it, the scaled gradient
 *   map, the six gradients and an optional Adam step on the device behind it; csrc/exposure.hip).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_frame_debug_tile_compact and
 *   gs_frame_debug_tile_cost (read-only views of two per-tile words of the last forward, for tests and measurements: the step
 *   at which a tile's compositing wave compacted its live pixels, and the steps it composited); the workspace of a frame grows
 *   by one word per tile (gs_frame_workspace_bytes).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_CULL_REPEAT (an
 *   occlusion-culled frame that repeats the previous one is issued without the five gated launches of its second pass) and
 *   gs_frame_cull_second_pass (does a forward of this descriptor enqueue them: host-side, no launch);
 *   gs_frame_debug_cut_table (a read-only view of the per-tile cuts, for tests).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_densify_apply_state (the arrays
 *   that share the row index with the Gaussians -- the optimizer's moments -- follow a densification: kept and cloned rows keep
 *   theirs, split rows, clones and second samples start from zero; gs_prune_arrays is reused, gs_densify_classify and
 *   gs_densify_apply are unchanged).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_DEVICE_POSE with
 *   gs_frame_dp -- a gs_frame_pp followed by pose_dev, 12 floats in device memory that the frame's kernels read as its pose,
 *   read only when the flag is set; gs_frame, gs_frame_scene and gs_frame_pp are unchanged --, honoured by gs_frame_forward and
 *   gs_frame_backward_pose; gs_pose_step, gs_pose_reset and gs_pose_log_bytes with gs_pose_state / gs_pose_step_opts /
 *   GS_POSE_LOG_HEAD (Adam on the pose's six tangent numbers on the device, one launch per iteration: camera tracking
 *   without a host read inside the loop).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_view_redundancy,
 *   gs_view_redundancy_pp and gs_view_redundancy_workspace_bytes with GS_REDUNDANCY_BINS (of the surface points one keyframe
 *   measured, how many are seen by 0, 1, ..., 7 or more of the OTHER keyframes: the measurement behind keyframe eviction).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_icp_model_maps, gs_icp_step and
 *   gs_icp_reset with gs_icp_model_opts / gs_icp_opts / gs_icp_state and the size queries gs_icp_model_bytes,
 *   gs_icp_workspace_bytes and gs_icp_log_bytes (frame-to-model point-to-plane ICP of a range map against the map's vertex and
 *   normal maps: association, normal equations and the 6 x 6 solve on the device, no host read inside the loop).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_track_gate_mask +
 *   gs_track_gate_mask_workspace_bytes (the median gate of gs_loss_track_gated as a keyframe's mapping inputs: a range map
 *   without the rejected measurements and a per-pixel colour weight) and gs_loss_l1_ssim_weighted (gs_loss_l1_ssim with a
 *   per-pixel weight map).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_pyramid_down with
 *   gs_pyramid_opts / GS_PYRAMID_MAX_LEVELS (one level down of an image pyramid -- box-filtered colour and a measurement-aware
 *   range map -- in one launch: the level targets of coarse-to-fine camera tracking).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_PRINCIPAL_POINT with
 *   gs_frame_pp -- a gs_frame_scene followed by pp_dx / pp_dy, the principal point's offset in pixels from the renderer's centre,
 *   read only when the flag is set; gs_frame and gs_frame_scene are unchanged --, honoured by every gs_frame_* entry point;
 *   gs_seed_camera_pp (a gs_seed_camera followed by the same two offsets; gs_seed_camera stays 64 bytes) with gs_seed_apply_pp
 *   and gs_view_overlap_pp, the variants of gs_seed_apply and gs_view_overlap for cameras with an off-centre principal point.
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_prune_workspace_bytes,
 *   gs_prune_classify and gs_prune_apply with gs_prune_opts / gs_prune_arrays / GS_PRUNE_MAX_ARRAYS (remove Gaussians by one
 *   per-row decision and move every array that shares the row index -- parameters, optimizer moments, the densification
 *   statistic -- in one stable compaction).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_frame_backward_pose (the pose
 *   gradient of a GS_FRAME_POSE_GRAD frame alone, without any per-Gaussian gradient: camera tracking against a frozen map).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_frame_backward_adam_pose (the
 *   fused training step for GS_FRAME_POSE_GRAD frames, with or without GS_FRAME_AUX: the pose gradient of a mapping step).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_view_overlap,
 *   gs_view_overlap_workspace_bytes and gs_view_overlap_check_view with gs_overlap_opts / GS_OVERLAP_MAX_VIEWS (how many of the
 *   surface points an RGB-D frame measured does each keyframe see: the covisibility count of a mapping loop).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_loss_track_gated +
 *   gs_loss_track_gated_workspace_bytes (gs_loss_track with each term gated at a multiple of the frame's own median
 *   residual: an exact device radix select, no host synchronisation).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_loss_track +
 *   gs_loss_track_workspace_bytes (the masked colour + depth loss of camera tracking against a frozen map, one pass).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_seed_workspace_bytes,
 *   gs_seed_classify and gs_seed_apply with gs_seed_opts / gs_seed_camera (new Gaussians from an RGB-D frame by
 *   back-projection of the measured pixels the current model does not explain).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): gs_loss_depth +
 *   gs_loss_depth_workspace_bytes (L1 depth supervision on the GS_FRAME_AUX maps) and gs_frame_backward_adam_aux (the fused
 *   training step for GS_FRAME_AUX frames).
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_SCENE_PACK with
 *   gs_frame_scene -- a gs_frame followed by scene_pack_a / scene_pack_b / scene_pack_a_bytes / scene_pack_b_bytes, read only
 *   when the flag is set; gs_frame itself is unchanged --, gs_scene_pack_bytes, gs_scene_pack_build and
 *   gs_frame_reads_scene_pack.
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_POSE_GRAD with the
 *   trailing gs_frame fields grad_rot / grad_tran / pose_workspace / pose_workspace_bytes (behind the GS_FRAME_AUX fields,
 *   read only when the flag is set) and gs_frame_pose_workspace_bytes.
 * 8, purely additive (clients built against the earlier version 8 header are unaffected): GS_FRAME_AUX with the trailing
 *   gs_frame fields depth / alpha / aux_padded / aux_workspace / aux_workspace_bytes / grad_depth / grad_alpha (read only
 *   when the flag is set) and gs_frame_aux_workspace_bytes.
 * 8 (round 6): gs_frame_is_occlusion_culled; an occlusion-culled frame's first pass projects only the Gaussians that are not
 * behind every cut they can reach and writes rectangle records for those only.
 *   GS_FRAME_CULL_DILATE.
 * 7 (round 6): GS_FRAME_LONG_SORT, GS_FRAME_OCCLUSION_CULL + gs_frame_cull_fallback_async; gs_frame_stats_serial (the frame the
 * counters belong to).
 * 6 (round 5): gs_frame_backward_adam (the backward with the optimizer step fused in); gs_frame_debug_bwd_exec_rows; GS_FRAME_BWD_ROWS and the saturated-bucket count in the upper half of the
 * `buckets` counter; SH gradient rows in whole 64-byte lines without per-row flags (workspace
 * layout only: no signature changed).
 * 5 (round 4): the frame in pieces -- gs_frame_forward_project + gs_frame_forward_rest == gs_frame_forward,
 * gs_frame_backward_slice (the per-Gaussian sums of a range of Gaussians), gs_frame_project_slices --, gs_adam_step_multi /
 * gs_adam_step_range (up to eight element ranges per launch, grad_scale), gs_grad_stat_update, gs_frame_longest_list_async.
 * 4 (round 3): GS_FRAME_STRIP_BIN + the size-based choice of the binning variant, gs_frame_binning_variant,
 * gs_frame_debug_rects (records of culled Gaussians are no longer written), gs_frame_overflow_flag,
 * gs_adam_step_sharded, `fast = 0` of gs_draw / gs_draw_backward honoured, the long-list kernels follow GS_FRAME_LONG_LISTS alone (not the
 * workspace capacity).  3: gs_frame.async / flags. */
#define GS_ABI_VERSION 8

#define GS_E_INVALID (-1)   /* bad argument (null pointer, negative size, bad enum)   */
#define GS_E_UNSUPPORTED (-2) /* a valid request this entry point does not implement (gs_frame_backward_adam of a
                                 GS_FRAME_AUX frame -- gs_frame_backward_adam_aux takes those -- or of a
                                 GS_FRAME_POSE_GRAD frame -- gs_frame_backward_adam_pose takes those --; gs_frame_backward_slice of a
                                 GS_FRAME_POSE_GRAD frame; any backward of a GS_FRAME_POSE_GRAD frame with SH colours) */
#define GS_E_CAPACITY (-3)  /* workspace too small for this frame                     */

typedef void *gs_stream_t;

const char *gs_last_error(void);
int gs_abi_version(void);

/* =========================================================================================
 * A. The reference `gaussian` module surface (src/bindings.cpp:21-50)
 * ======================================================================================= */

/* bindings.cpp:23 `culling` -> gaussian.cu:6-8: a stub that prints "hellow". Kept as a no-op. */
int gs_culling(void);

/* bindings.cpp:24 `world2camera(pos, rot, trans, res)` -> gaussian.cu:49-76.
 * res[i] = rot * pos[i] + tran.   pos,res: [B,3]; rot: [3,3]; tran: [3]. */
int gs_world2camera(const float *pos, const float *rot, const float *tran, float *res, int64_t B,
                    gs_stream_t stream);

/* bindings.cpp:25 `world2camera_backward(grad_out, rot, grad_inp)` -> gaussian.cu:78-99. */
int gs_world2camera_backward(const float *grad_out, const float *rot, float *grad_inp, int64_t B,
                             gs_stream_t stream);

/* bindings.cpp:26 `jacobian(pos_camera_space, jacobian)` -> gaussian.cu:10-47.  jac: [B,3,3]. */
int gs_jacobian(const float *pos_cam, float *jac, int64_t B, gs_stream_t stream);

/* bindings.cpp:48 `global_culling` -> gaussian.cu:1182-1369.
 * pos [N,3], quat [N,4] (pre-normalised), scale [N,3] (pre-activated), rot [3,3], tran [3]
 * -> res_pos [N,3] = (x/z, y/z, |p_c|), res_cov [N,2,2], culling_mask [N] int64.
 * Rows of culled Gaussians are left untouched (the caller pre-zeroes, renderer.py:124-126). */
int gs_global_culling(const float *pos, const float *quat, const float *scale, const float *rot,
                      const float *tran, int64_t N, float near_plane, float half_width,
                      float half_height, float *res_pos, float *res_cov, int64_t *culling_mask,
                      gs_stream_t stream);

/* bindings.cpp:49 `global_culling_backward` -> gaussian.cu:1371-1609. */
int gs_global_culling_backward(const float *pos, const float *quat, const float *scale,
                               const float *rot, const float *tran, int64_t N,
                               const float *gradout_pos, const float *gradout_cov,
                               const int64_t *culling_mask, float *gradinput_pos,
                               float *gradinput_quat, float *gradinput_scale, gs_stream_t stream);

/* bindings.cpp:44 `calc_tile_list(Gaussian3ds&, Tiles&, tile_n_point, tile_gaussian_list,
 * thresh, method, tile_length_x, tile_length_y, n_tiles_x, n_tiles_y, leftmost, topmost)`
 * -> gaussian.cu:101-335.  The two structs are flattened: Gaussian3ds contributes pos [V,3]
 * and cov [V,2,2]; Tiles contributes top/bottom/left/right [T] (read by methods 0 and 1 only,
 * may be NULL for method 2).  tile_n_point [T] int32 must be zeroed by the caller;
 * tile_gaussian_list is [T, max_points_per_tile] int32.  Race-free: a tile keeps the first
 * `max_points_per_tile` arrivals, the counter keeps counting (the caller clamps it,
 * splatter.py:586). */
int gs_calc_tile_list(const float *pos, const float *cov, int64_t n_point, const float *tile_top,
                      const float *tile_bottom, const float *tile_left, const float *tile_right,
                      int32_t *tile_n_point, int32_t *tile_gaussian_list,
                      int64_t max_points_per_tile, float thresh, int method, float tile_length_x,
                      float tile_length_y, int32_t n_tiles_x, int32_t n_tiles_y, float leftmost,
                      float topmost, gs_stream_t stream);

/* bindings.cpp:45 `gather_gaussians(tile_n_point_accum, tile_gaussian_list, gathered_list,
 * tile_ids_for_points, max_points_for_tile)` -> gaussian.cu:337-381. */
int gs_gather_gaussians(const int32_t *tile_n_point_accum, const int32_t *tile_gaussian_list,
                        int32_t *gathered_list, int32_t *tile_ids_for_points, int64_t n_tiles,
                        int64_t max_points_for_tile, int64_t list_row_size, gs_stream_t stream);

/* bindings.cpp:46 `draw` -> gaussian.cu:806-1043.
 * pos [M,3] (z ignored), rgb [M,D] (D = 3, or 27 when use_sh_coeff), opa [M], cov [M,2,2],
 * tile_n_point_accum [T+1] int32, res [h,w,3] with h,w the PADDED size (multiples of 16).
 * rays_o/lefttop_pos/vec_dx/vec_dy: device float[3], only read when use_sh_coeff.
 * fast != 0: the Gaussian's value through the hardware exponential on a conic hoisted out of the pixel loop (the
 * reference's __expf flavour, gaussian.cu:920); fast == 0: the reference's exp() flavour (gaussian.cu:922-923): the
 * numerator as float products in its order, a double division by 2 det + 1e-14 and a double exp per pixel. */
int gs_draw(const float *pos, const float *rgb, const float *opa, const float *cov,
            const int32_t *tile_n_point_accum, float *res, int32_t h, int32_t w, int64_t M,
            float focal_x, float focal_y, int weight_normalize, int sigmoid, int fast,
            const float *rays_o, const float *lefttop_pos, const float *vec_dx,
            const float *vec_dy, int use_sh_coeff, gs_stream_t stream);

/* bindings.cpp:47 `draw_backward` -> gaussian.cu:440-803, 1045-1129.
 * grad_pos [M,3] (column 2 is never written), grad_rgb [M,D], grad_opa [M], grad_cov [M,2,2]:
 * one row per (tile, Gaussian) pair.  `workspace` holds the per-bucket pixel checkpoints of
 * the replayed forward pass: gs_draw_backward_workspace_bytes(M, h, w) bytes. */
size_t gs_draw_backward_workspace_bytes(int64_t M, int32_t h, int32_t w);
int gs_draw_backward(const float *pos, const float *rgb, const float *opa, const float *cov,
                     const int32_t *tile_n_point_accum, const float *output,
                     const float *grad_output, float *grad_pos, float *grad_rgb, float *grad_opa,
                     float *grad_cov, int32_t h, int32_t w, int64_t M, float focal_x,
                     float focal_y, int weight_normalize, int sigmoid, int fast,
                     const float *rays_o, const float *lefttop_pos, const float *vec_dx,
                     const float *vec_dy, int use_sh_coeff, void *workspace,
                     size_t workspace_bytes, gs_stream_t stream);

/* =========================================================================================
 * B. Fused frame path (replaces splatter.py:513-655 forward and its autograd backward)
 * ======================================================================================= */

/* Device radix sort of (key, value) pairs on key bits [0, end_bit), stable, ascending (LSD,
 * 8 bits per pass).  The element count is read from DEVICE memory (*d_count, clamped to
 * `capacity`) so that the frame needs no host synchronisation.  The input lives in buffer 0
 * (keys0/vals0, destroyed); buffer 1 is scratch; on return *sorted_in_buffer1 tells which
 * buffer holds the result (it only depends on end_bit).  tmp: gs_sort_pairs_tmp_bytes(capacity). */
size_t gs_sort_pairs_tmp_bytes(int64_t capacity);
int gs_sort_pairs(uint64_t *keys0, uint32_t *vals0, uint64_t *keys1, uint32_t *vals1,
                  const uint32_t *d_count, int64_t capacity, int end_bit, void *tmp,
                  size_t tmp_bytes, int *sorted_in_buffer1, gs_stream_t stream);
/* Same, restricted to key bits [begin_bit, end_bit): a stable partial sort (used by sort_mode 1
 * to group pairs by tile id only). */
int gs_sort_pairs_bits(uint64_t *keys0, uint32_t *vals0, uint64_t *keys1, uint32_t *vals1,
                       const uint32_t *d_count, int64_t capacity, int begin_bit, int end_bit,
                       void *tmp, size_t tmp_bytes, int *sorted_in_buffer1, gs_stream_t stream);

#define GS_FRAME_EMIT_SORTED_KEYS 1 /* sort_mode 2: also write the sorted (tile << 32 | depth bits) keys that
                                       gs_frame_debug_views returns (modes 0 / 1 always have them); the raster
                                       kernels only read the sorted ids, so the default path skips 8 bytes per pair */

#define GS_FRAME_SLICE_SORT 2       /* sort_mode 2: the slice-sorted binning variant (tile_bin.hip) -- every workgroup
                                       counting-sorts the pairs of its slice of the Gaussians by tile inside LDS and
                                       streams them out contiguously, the per-tile sort gathers from the slices.  No
                                       scattered global store, but one small (slice, tile) cell per gather step:
                                       measured slower than the table variant up to 2.4 M Gaussians at 1080p
                                       (DESIGN.md), so it is opt-in.  Same result either way. */

#define GS_FRAME_TABLE_BIN 4        /* sort_mode 2: the table variant (tile_bin.hip: count -> column scan -> one scattered
                                       8-byte store per pair) instead of the default two-level STRIP variant
                                       (strip_bin.hip).  Frames beyond the strip variant's limits (2^26 Gaussians, 8192
                                       strips of 8 tiles) take the table variant by themselves.  Same result. */

#define GS_FRAME_SERIAL_LONG_LISTS 8 /* dense frames (capacity above 1024 pairs per tile on average) cut the rest of a tile's
                                       list into segments composited by many waves when its pixels are still alive after
                                       4096 Gaussians (raster_fwd_segment.hip); this flag keeps the one-wave-per-tile walk for
                                       such tiles (A/B and equivalence tests).  Same result up to the rounding of the
                                       transmittance entering a segment. */

#define GS_FRAME_LONG_LISTS 16       /* run the long-list kernels (big-list sort, segmented compositing): for dense scenes (10 M
                                       Gaussians at 1080p: ~3,500 pairs per tile) and for frames that hold a few very
                                       long lists (pile-ups of a degenerate densification run).  The library cannot know
                                       without a host synchronisation; the caller can: gs_frame_longest_list_async
                                       reports the longest list of an earlier frame.  A frame without the flag is
                                       correct whatever its lists are, only slower on long ones; the workspace CAPACITY
                                       never selects the path (up to ABI version 3 a capacity above 1024 pairs per tile
                                       did). */

#define GS_FRAME_STRIP_BIN 32        /* sort_mode 2: take the strip variant of the binning whatever the scene size.  Without
                                       this flag (and without GS_FRAME_TABLE_BIN / GS_FRAME_SLICE_SORT) the library picks
                                       by N: the table variant below GS_STRIP_AUTO_MIN_N (131,072) Gaussians, where its shorter
                                       chain of dependent kernels wins, the strip variant from there on.  Every variant
                                       produces the same lists. */
#define GS_FRAME_LONG_SORT 128        /* the SORT half of GS_FRAME_LONG_LISTS alone (round 6): tile lists beyond strip_sort_kernel's LDS
                                       window (2,048 pairs) are queued for big_list_sort_kernel, one workgroup per list, instead
                                       of being sorted by their strip's workgroup with the chunked bitonic network -- the tail of
                                       that kernel in a trained / densified scene (3.9 M pairs, 165 lists beyond 2,048: per-tile
                                       sort 407 -> 122 us, profiles/r06_a_*).  The sorted list is the same either way (the order is
                                       exact), so unlike the segmented compositing this half costs nothing but two launches in
                                       frames without such lists.  The caller sets it once gs_frame_longest_list_async reported
                                       a list beyond 2,048; GS_FRAME_LONG_LISTS implies it. */
#define GS_FRAME_OCCLUSION_CULL 256   /* temporal occlusion cull (round 6): allow the frame to drop, at emission, the (tile, Gaussian)
                                       pairs that lie behind the depth at which the PREVIOUS forward of this workspace saw all
                                       pixels of their tile stop -- 71 % of the pairs of the 2.4 M-Gaussian scene are emitted,
                                       scattered and sorted and never composited.  The image is exact (bit-identical to the
                                       unculled frame) whatever the camera or the scene did since: a tile's trimmed list is
                                       every pair up to its cut plus some of the deeper ones (runs are trimmed at their ends
                                       only), and a tile that composites anything behind its cut -- or reaches the end of
                                       its trimmed list with a live pixel -- makes the library render the frame
                                       again from the full lists, on the device, inside the same call (five gated launches:
                                       8.6 us of a 215-us frame when nothing ran past its cut -- GS_FRAME_CULL_REPEAT leaves them
                                       out where they cannot run --; 0.6 of a frame when something did, which with thousands
                                       of tiles is nearly every frame of a MOVING camera: set the flag for a camera at rest).  The CALLER's promise: the previous
                                       forward of this workspace was an inference frame (training = 0: training forwards do
                                       not write the table) of the same width and height (the cut table is per tile).
                                       Ignored by training frames, frames with GS_FRAME_EMIT_SORTED_KEYS / GS_FRAME_LONG_LISTS /
                                       GS_FRAME_SERIAL_LONG_LISTS, the "dist" listing and the table / radix variants.
                                       gs_frame_stats_async then reports the pairs that were emitted (fewer than the frame
                                       lists); gs_frame_cull_fallback_async tells whether the frame was re-rendered. */
#define GS_FRAME_CULL_DILATE 512      /* with GS_FRAME_OCCLUSION_CULL: every tile's cut is the LARGEST cut of its 3 x 3 tile
                                       neighbourhood (no cut if one of the nine has none), pushed back by a factor 1.375 in depth
                                       -- for a camera that has MOVED by less than half a tile since the table was recorded.  On
                                       the 2.4 M-Gaussian scene no frame of a 1.25-pixel-per-frame pan falls back (3 of 119 at
                                       5 px per frame), 3.1 M of 6.95 M pairs are emitted (1.8 M with the tiles' own cuts, which
                                       fit the identical pose only): +20 % FPS.  The image is exact either way (the second pass).
                                       One more launch of ~2 us. */
#define GS_FRAME_CULL_DILATE_NEAR 1024 /* with GS_FRAME_CULL_DILATE: the pose is within half a pixel of the recorded one (what a viewer
                                       in motion produces at thousands of frames per second): depth factor 1.125 instead of
                                       1.375 -- 2.5 M instead of 3.1 M of 6.95 M pairs emitted, no fallback over a 0.25-px/frame pan */
#define GS_FRAME_BWD_ROWS 64         /* rgb training frames: composite the backward with the row-layout kernel (lanes = 16
                                       Gaussians x 4 pixel quads, pixel rows whose pixels have all stopped are left out)
                                       instead of the pixel-parallel one.  Worth it when most of the frame's buckets belong
                                       to SATURATED tiles -- tiles whose compositing stopped before the end of their list --
                                       and a loss otherwise (2.4 M Gaussians at 1080p: -9 %; 376 k Gaussians: +11 %, kernel
                                       traces profiles/r05_e_*).  The library cannot know without a host synchronisation;
                                       the caller can: the upper half of gs_frame_stats_async's `buckets` counter is the
                                       number of buckets of saturated tiles in the last backward's work list.  Either
                                       kernel is correct for any frame; the results differ in the last bits (another
                                       summation order).  Ignored by SH frames. */

#define GS_FRAME_AUX 2048             /* the frame also renders two per-pixel maps over exactly the Gaussians the colour composites
                                       (up to the same 1e-4 stop), cropped like the image and NOT clamped:
                                         alpha[H,W] = sum_i w_i            (accumulated like a colour channel of value 1.0;
                                                                            = 1 - the final transmittance)
                                         depth[H,W] = sum_i w_i d_i        d_i = |p_c|, the distance from the camera centre
                                                                            (rec_geom.z, the key the lists are sorted by --
                                                                            not camera z)
                                       with w_i = alpha_i T_i.  The expected depth is depth / alpha (left to the caller).
                                       Every colour model, training and inference frames; the trailing fields of gs_frame
                                       below carry the buffers.  Training frames: gs_frame_backward / _part / _slice take
                                       grad_depth / grad_alpha as well, and so does the fused training step
                                       gs_frame_backward_adam_aux (gs_frame_backward_adam itself refuses the frame:
                                       GS_E_UNSUPPORTED).  Such frames walk every tile list with one wave (no segmented
                                       compositing of long lists, as with GS_FRAME_SERIAL_LONG_LISTS: the same result,
                                       slower on very long lists only), and their backward composites on the
                                       one-wave-per-bucket pixel kernel for every colour model (not the row-layout rgb
                                       kernel, not the matrix pipe).  Frames without the flag run exactly the kernels
                                       they ran before it existed. */

#define GS_FRAME_POSE_GRAD 4096       /* the backward also writes the gradient of the loss with respect to the camera pose:
                                         grad_rot[3,3] = dL/d(rot) (row-major, the Euclidean gradient in the nine entries:
                                                         not projected onto SO(3) -- parametrise the rotation upstream),
                                         grad_tran[3]  = dL/d(tran),
                                       with p_c = rot p + tran.  The projection Jacobian J of cov2d = J rot C rot^T J^T is
                                       held fixed, as for every per-Gaussian gradient of this library (and the reference's
                                       global_culling_backward): the pose gradient is exactly the one the per-Gaussian
                                       gradients imply -- moving the camera is moving every Gaussian the other way --, so a
                                       joint pose + scene fit stays consistent.  Per visible Gaussian, gc = dL/dp_c:
                                         dL/dtran += gc,  dL/drot += gc p^T + J^T (G + G^T) J rot C,  G = dL/dcov2d;
                                       with GS_FRAME_AUX the depth map's term (gc = g_d p_c / |p_c|) counts as well.
                                       Culled Gaussians contribute nothing; a frame with N = 0 or one that overflowed its
                                       workspace (rendered empty) gets zeros.  Both are written (overwritten, never
                                       accumulated) by gs_frame_backward, gs_frame_backward_profile and
                                       gs_frame_backward_part(GS_BWD_GEOMETRY); GS_BWD_RASTER / GS_BWD_COLOR leave them
                                       alone, forwards ignore the flag apart from validating the fields.  The sum runs in a
                                       fixed order without atomics: bitwise repeatable.
                                       rgb colours only (color_dim 3): with SH colours the image also depends on the pose
                                       through each pixel's ray direction, which is not differentiated -- every backward of
                                       such a frame returns GS_E_UNSUPPORTED.  gs_frame_backward_slice returns
                                       GS_E_UNSUPPORTED (a frame in slices has no point at which all partial sums are in)
                                       and so do gs_frame_backward_adam and gs_frame_backward_adam_aux: the fused training
                                       step of a flagged frame is gs_frame_backward_adam_pose, which writes both as well.
                                       gs_frame_backward_pose writes both and nothing else: the same bits without the
                                       per-Gaussian gradients, for a caller that holds the map fixed.
                                       All refusals come before anything is enqueued.
                                       Frames without the flag run exactly the kernels they ran before it existed. */

#define GS_FRAME_SCENE_PACK 8192      /* the frame carries a SCENE PACK (the descriptor is a gs_frame_scene, below: built by
                                       gs_scene_pack_build): the camera-independent half of the projection of every Gaussian
                                       -- activations, R S S R^T, the activated opacity and rgb colour, 80 bytes per Gaussian
                                       (192 MB at 2.4 M) --, which the project stage of an inference frame of the strip
                                       variant then reads INSTEAD of the raw arrays.  The frame is bit for bit the frame
                                       rendered without the flag: the same expressions on the same inputs in the same
                                       order, half of them evaluated once instead of once per frame.
                                       THE CALLER PROMISES that the pack was built from exactly the arrays this frame names
                                       (pos, quat, scale, opa, rgb, N), with this frame's color_dim and scale_activation, and
                                       that none of the arrays has been written since.  The library cannot check it (the
                                       check would be the pass over memory the pack removes), and unlike a stale cut table
                                       of GS_FRAME_OCCLUSION_CULL, which costs a second pass, a stale pack renders a WRONG
                                       IMAGE.  The raw arrays must still be valid: the paths below read them.
                                       GS_E_INVALID, before anything is enqueued, for a flagged training frame, a NULL
                                       plane, a plane shorter than gs_scene_pack_bytes says, scene_pack_a not 16-byte or
                                       scene_pack_b not 64-byte aligned.  Ignored (the raw arrays are read) by the table /
                                       slice-sorted / radix variants and by gs_frame_forward_project's frames, which are
                                       training frames; gs_frame_reads_scene_pack tells.  Frames without the flag run
                                       exactly the kernels they ran before it existed. */

#define GS_FRAME_PRINCIPAL_POINT 16384 /* the camera's principal point is NOT the renderer's centre (the descriptor is a gs_frame_pp,
                                       below).  The centre: pixel (i, j) of the width x height image covers [i, i + 1) x [j, j + 1)
                                       (COLMAP's convention) and the optical axis of an unflagged frame passes through
                                       cx0 = padW / 2 - (padW - width) / 2 (integer division: width / 2 for an even width,
                                       (width + 1) / 2 for an odd one), cy0 likewise.  pp_dx = cx - cx0, pp_dy = cy - cy0.
                                       The tile grid, the padded image and the centred crop are those of the unflagged frame;
                                       the offset enters at ONE place, the projected centre of a Gaussian, in fp32 with one
                                       rounding per operation:
                                         sx = (float)(pp_dx / focal_x), sy = (float)(pp_dy / focal_y)     (host, in double)
                                         pos_i = (fl(fl(x / z) + sx), fl(fl(y / z) + sy), |p_c|)
                                         culled <=> z <= near or |pos_i.x| >= half_width or |pos_i.y| >= half_height
                                       -- the frustum test looks at the SHIFTED centre: the guard band stays centred on the
                                       image.  Binning, sorting, compositing, the maps and every backward read that centre;
                                       the Jacobian, the covariance, the projection backward and the pose gradient are
                                       functions of p_c and are unchanged (a constant added to pos_i has derivative 1).  SH
                                       colours: the caller's ray basis moves with the principal point, lefttop_cam =
                                       ((-padW / 2 + 0.5 - pp_dx) / focal_x, (-padH / 2 + 0.5 - pp_dy) / focal_y, 1).
                                       Every gs_frame_* entry point honours the flag, with or without a scene pack (the pack
                                       is camera-independent).  An offset of exactly (0, 0) runs the unflagged frame's code
                                       paths and gives its bits.  GS_E_INVALID, before anything is enqueued, for an offset
                                       that is not finite (or beyond 1e6 pixels) or a non-positive focal length.  Frames
                                       without the flag run exactly the code paths they ran before it existed. */

#define GS_FRAME_DEVICE_POSE 32768    /* the frame's pose is READ FROM DEVICE MEMORY (the descriptor is a gs_frame_dp, below):
                                       pose_dev points to 12 floats, rot[9] row-major then tran[3], 16-byte aligned, and the
                                       frame's kernels take rot / tran from it AS IT STANDS WHEN THEY EXECUTE -- a pose that an
                                       earlier kernel on the stream wrote (gs_pose_step) needs no host round trip.  f->rot /
                                       f->tran are still held to the descriptor's rules, but no kernel of a flagged frame reads
                                       them.  The same expressions run on the same numbers: a flagged frame is the by-value
                                       frame of that pose bit for bit, forward and backward.
                                       THE CALLER PROMISES that the 12 floats do not change between a flagged forward and its
                                       backward (the backward would differentiate another frame than the one rendered).
                                       Honoured by gs_frame_forward and gs_frame_backward_pose (part 0 and GS_BWD_GEOMETRY);
                                       the counter, overflow, variant and size queries ignore the pose.  GS_E_INVALID, before
                                       anything is enqueued, for a null or misaligned pose_dev; else GS_E_UNSUPPORTED, before
                                       anything is enqueued, for a flagged frame that is not a training frame, has SH colours
                                       (rays_o / lefttop / vec_dx / vec_dy are pose-derived host scalars), sort_mode 0 or 1
                                       (as given or as the library would pick for the grid), GS_FRAME_OCCLUSION_CULL or
                                       GS_FRAME_SCENE_PACK, and from every other entry point that launches: gs_frame_backward,
                                       _part, _slice, _profile, the fused Adam backwards, gs_frame_forward_project / _rest /
                                       _profile, gs_frame_contrib and the debug views.  Frames without the flag run exactly
                                       the kernels they ran before it existed. */

#define GS_FRAME_CULL_REPEAT 65536    /* with GS_FRAME_OCCLUSION_CULL: this frame REPEATS the previous forward of its workspace, and
                                       the library does not enqueue the five gated launches of the second pass behind it.
                                       Nothing else changes: the first pass trims by the recorded cuts, the compositing
                                       epilogue compares against them and raises the run-past counter, the cut table, the
                                       tile costs and every counter are written as in any culled frame.
                                       THE CALLER PROMISES that (1) the previous forward of this workspace used this
                                       descriptor field for field, the output pointers (image, image_padded, depth, alpha)
                                       aside; (2) the scene bytes the two frames read -- the raw arrays or the scene pack --
                                       are the same; (3) a culled frame (GS_FRAME_OCCLUSION_CULL without
                                       GS_FRAME_CULL_DILATE) with exactly these inputs has been seen to finish with the
                                       run-past counter at 0 (gs_frame_cull_fallback_async, or [10] and, for the capacity,
                                       [2] of gs_frame_stats_tagged_async).
                                       Why that is enough: at an unchanged pose and scene a tile stops
                                       at the Gaussian that set its cut, so the depth test of the epilogue never fires and the
                                       frame writes the cut table it read; the one other source of a run-past, a slice
                                       that overflows its staging region, depends on entry counts alone, which identical
                                       inputs reproduce whatever the order of the LDS adds.  A frame with identical inputs
                                       therefore runs past if and only if the one before it did.
                                       What a client tracks to make the promise: the pose and intrinsics by value, every
                                       other descriptor field, the workspace (address, size, max_pairs), and the CONTENTS of
                                       the scene -- not its address alone: an in-place edit, or a freed array whose address
                                       comes back, breaks (2) -- and it drops the promise until it holds fresh evidence (3)
                                       whenever one of them changes or another forward used the workspace in between.
                                       The check after the fact is complete: for ANY cut table, a culled frame that ends with
                                       the run-past counter at 0 is the unculled frame bit for bit.  A flagged frame has the
                                       counter at 0 and is exact, or at 1 and the caller can know it for certain
                                       (gs_frame_cull_fallback_async): no silent third case.  A non-zero counter on a
                                       flagged frame means the promise was broken, the frame was NOT rendered again and the
                                       image delivered is not guaranteed; the next forward without this flag is repaired
                                       as usual.
                                       Ignored wherever GS_FRAME_OCCLUSION_CULL is ignored (no second pass exists there).
                                       GS_E_INVALID, before anything is enqueued, together with GS_FRAME_CULL_DILATE: dilated
                                       cuts belong to a camera that moved, which contradicts (1).  gs_frame_cull_second_pass
                                       tells, without a launch, whether a forward enqueues the gated launches.
                                       gs_frame_forward_profile honours the flag: the "total" of a flagged frame closes behind
                                       the compositing launch. */

/* Frame descriptor.  All scalars are per-camera constants computed on the host exactly as
 * splatter.py does (Tiles, RayInfo, frustum guard band); rot/tran are passed by value. */
typedef struct gs_frame {
    /* scene (raw parameters, activations are fused: |s|+1e-4 / exp, q/|q|, sigmoid) */
    int64_t N;
    int32_t color_dim;        /* 3 (sigmoid colour), 27 (degree-2 SH coefficients, the reference's basis_dim 9) or
                                 48 (degree-3 SH: extension with the C3 table of gaussian.cu:395-403) */
    int32_t scale_activation; /* 0 = abs (+1e-4), 1 = exp   (splatter.py:520-524)       */
    const float *pos;         /* [N,3]  */
    const float *quat;        /* [N,4]  */
    const float *scale;       /* [N,3]  */
    const float *opa;         /* [N]    */
    const float *rgb;         /* [N,color_dim] */
    /* camera */
    float rot[9];
    float tran[3];
    float near_plane, half_width, half_height;
    int32_t width, height;    /* un-padded output size */
    float focal_x, focal_y;
    /* Tiles.create_tiles scalars, computed by the host in double (splatter.py:279-282) */
    float tile_length_x, tile_length_y, leftmost, topmost;
    float thresh;             /* tile_culling_prob_thresh (train.py: 0.05) */
    float rays_o[3], lefttop[3], vec_dx[3], vec_dy[3];
    /* workspace (caller-allocated, sizes from gs_frame_workspace_layout) */
    int64_t max_pairs;        /* capacity for (tile, Gaussian) pairs                      */
    void *workspace;
    size_t workspace_bytes;
    /* outputs */
    float *image;             /* [height,width,3] clamped + cropped (may be NULL)         */
    float *image_padded;      /* [padH,padW,3] raw draw output (may be NULL if !training) */
    int32_t training;         /* 1: keep per-bucket checkpoints for gs_frame_backward      */
    int32_t sort_mode;        /* how the (tile, depth) order is produced -- same result either way:
                                 0 = LSD radix sort of 64-bit (tile<<32|depth) keys (gs_sort_pairs)
                                 1 = hybrid: stable LSD radix passes on the tile bits only (2 passes at
                                     1080p), then every tile's bucket sorted on (depth, id) in LDS
                                 2 = counting sort in LDS, no radix pass (default).  Strip variant: 8-byte
                                     entries per (Gaussian, strip of 8 tiles) counting-sorted by strip, expanded
                                     into the tile lists and depth-sorted inside LDS (up to 2^26 Gaussians and
                                     8192 strips; beyond that, or with GS_FRAME_TABLE_BIN: one LDS counter per
                                     tile, <= 32768 tiles, larger grids take mode 1).  On capacity overflow the
                                     frame is left empty (modes 0/1 keep the first max_pairs pairs); all modes
                                     report the true count in the stats. */
    int32_t tile_culling_method; /* which tiles a Gaussian is listed in (splatter.py:571-578, --tile_culling_method;
                                 the reference's own numbering, `_method_config` of splatter.py:571):
                                 2 = "prob2", the trainer's default (gaussian.cu:197-250: tile rectangle from the 2-D
                                     covariance's bounding box by index arithmetic);
                                 1 = "prob" (gaussian.cu:138-195: the same bounding box compared with the tiles'
                                     edges, Tiles.create_tiles of splatter.py:275-293 -- also a rectangle);
                                 0 = "dist" (gaussian.cu:101-136: every tile whose CENTRE lies closer than
                                     sqrt(thresh) to the Gaussian's centre, whatever its size).  `thresh` is then
                                     the squared distance (tile_length_x / tile_culling_dist_thresh)^2 of
                                     splatter.py:577; sort_mode 2 only (<= 32768 tiles).  The gradient rows are
                                     laid out over the bounding square of the disc, so max_pairs must cover the
                                     sum of those squares (reported as overflow otherwise). */
    /* ABI 3 */
    struct gs_frame_async *async; /* NULL, or a handle from gs_frame_async_create: training forwards then run the
                                 backward's preparation underneath the caller's loss (see gs_frame_forward) */
    int32_t flags;            /* GS_FRAME_* bits */
    /* GS_FRAME_AUX (read only when the flag is set; a client built against a header without these fields never sets it) */
    float *depth, *alpha;     /* [height,width] cropped maps (either may be NULL)                                      */
    float *aux_padded;        /* [padH,padW,2] raw (depth, alpha) sums; required when training (the backward reads it)  */
    void *aux_workspace;      /* caller-allocated, 256-byte aligned: gs_frame_aux_workspace_bytes(max_pairs, width,
                                 height, training) bytes, kept with `workspace` from the forward to its backward          */
    size_t aux_workspace_bytes;
    const float *grad_depth, *grad_alpha; /* backward inputs dL/d(depth), dL/d(alpha) [height,width]; NULL = zero           */
    /* GS_FRAME_POSE_GRAD (read only when the flag is set): device buffers, all required                                  */
    float *grad_rot;          /* [3,3] row-major: dL/d(rot)                                                                */
    float *grad_tran;         /* [3]: dL/d(tran)                                                                           */
    void *pose_workspace;     /* caller-allocated, 256-byte aligned: gs_frame_pose_workspace_bytes(N) bytes (per-workgroup
                                 partial sums; needed by the backward only, free between frames)                          */
    size_t pose_workspace_bytes;
} gs_frame;

/* GS_FRAME_SCENE_PACK: the descriptor of a flagged frame continues behind gs_frame with four more fields.  A caller that sets
 * the flag passes &s.frame of a gs_frame_scene to the entry points, all of which keep taking `const gs_frame *`; the library
 * reads the four fields only when the flag is set, which is the rule the GS_FRAME_AUX and GS_FRAME_POSE_GRAD fields follow.
 * They are a struct of their own and not members of gs_frame so that sizeof(gs_frame) and its last member stay what every
 * client of version 8 was built against. */
typedef struct gs_frame_scene {
    gs_frame frame;           /* first member: (const gs_frame_scene *)f == f                                              */
    const void *scene_pack_a; /* 16-byte aligned, >= a_bytes of gs_scene_pack_bytes(N, ...)                                 */
    const void *scene_pack_b; /* 64-byte aligned, >= b_bytes                                                                */
    size_t scene_pack_a_bytes, scene_pack_b_bytes;
} gs_frame_scene;

/* GS_FRAME_PRINCIPAL_POINT: the descriptor of a flagged frame continues behind gs_frame_scene with two more fields, by the
 * rule of gs_frame_scene: read only when the flag is set; the pack fields in front of them are read only with
 * GS_FRAME_SCENE_PACK and may be zero otherwise.  sizeof(gs_frame) and sizeof(gs_frame_scene) stay what they were. */
typedef struct gs_frame_pp {
    gs_frame_scene scene;     /* first member: (const gs_frame_pp *)f == f                                                  */
    double pp_dx, pp_dy;      /* cx - cx0, cy - cy0 in pixels (see the flag)                                               */
} gs_frame_pp;

/* GS_FRAME_DEVICE_POSE: the descriptor of a flagged frame continues behind gs_frame_pp with one more field, by the rule of
 * gs_frame_scene and gs_frame_pp: read only when the flag is set; the fields in front of it are read only with their own flags
 * and may be zero otherwise.  sizeof(gs_frame), sizeof(gs_frame_scene) and sizeof(gs_frame_pp) stay what they were. */
typedef struct gs_frame_dp {
    gs_frame_pp pp;           /* first member: (const gs_frame_dp *)f == f                                                  */
    const float *pose_dev;    /* DEVICE, 16-byte aligned: rot[9] row-major, tran[3] (see the flag)                          */
} gs_frame_dp;

/* Bytes of workspace needed for N Gaussians, `max_pairs` pairs, a width x height image. */
size_t gs_frame_workspace_bytes(int64_t N, int64_t max_pairs, int32_t width, int32_t height,
                                int32_t color_dim, int32_t training);

/* Bytes of aux workspace a GS_FRAME_AUX frame needs (host-only, no device call): the per-bucket (depth, alpha) checkpoints
 * of training frames (8 B x 256 pixels x the bucket capacity of `max_pairs` pairs) and a small header.  0 on bad arguments.
 * The main workspace (gs_frame_workspace_bytes) and its layout are the same with or without the flag. */
size_t gs_frame_aux_workspace_bytes(int64_t max_pairs, int32_t width, int32_t height, int32_t training);

/* Bytes of pose workspace a GS_FRAME_POSE_GRAD frame of N Gaussians needs (host-only, no device call): one row of 12 floats
 * per 256 Gaussians for the projection backward and one for the aux depth backward, and a small header.  0 when N < 0. */
size_t gs_frame_pose_workspace_bytes(int64_t N);

/* Scene pack (GS_FRAME_SCENE_PACK).  gs_scene_pack_bytes: bytes of the two planes for N Gaussians (host-only): 16 N and 64 N,
 * each rounded up to 256; returns their sum, 0 (and zeros) when N < 0; either out pointer may be NULL.
 * gs_scene_pack_build: writes both planes from the raw arrays on `stream` (one kernel, 56 B in and 80 B out per Gaussian); pack_a
 * 16-byte, pack_b 64-byte aligned, of at least those sizes.
 * gs_frame_reads_scene_pack (host-only): 1 exactly when the frame AS DESCRIBED, flagged or not, is one whose project stage would
 * read a pack -- an inference frame of the strip variant with N > 0 --, else 0 (also for a NULL frame): a caller need not build
 * 80 bytes per Gaussian for a frame that would ignore them. */
size_t gs_scene_pack_bytes(int64_t N, size_t *a_bytes, size_t *b_bytes);
int gs_scene_pack_build(const float *pos, const float *quat, const float *scale, const float *opa, const float *rgb, int64_t N,
                        int32_t color_dim, int32_t scale_activation, void *pack_a, void *pack_b, gs_stream_t stream);
int gs_frame_reads_scene_pack(const gs_frame *f);

/* Forward frame.  Launches everything on `stream`, never synchronises, and keeps no state of its own.
 * With f->training AND f->async the zero-fill of the per-pair gradient rows and the backward's bucket list are
 * issued on the handle's side stream, which waits for the frame's last kernel, so that they run underneath whatever
 * the caller enqueues between forward and backward (the loss); gs_frame_backward -- from any host thread -- and the
 * next gs_frame_forward with the same handle wait for that stream's event.  Without a handle (or while `stream` is
 * being captured into a graph) the backward prepares inline. */
int gs_frame_forward(const gs_frame *f, gs_stream_t stream);

/* The opt-in side stream: a caller-owned handle (one per workspace in use) holding a non-blocking stream and two
 * events on the current device.  The library keeps nothing else between calls.
 *   gs_frame_async_wait    : make `stream` wait for side-stream work that may still be writing into the workspace of
 *                            the handle's last training forward -- call it before freeing or re-purposing that
 *                            workspace if no gs_frame_backward / gs_frame_forward followed the frame;
 *   gs_frame_async_destroy : releases the handle (work already queued still completes). */
typedef struct gs_frame_async gs_frame_async;
int gs_frame_async_create(gs_frame_async **out);
int gs_frame_async_wait(gs_frame_async *a, gs_stream_t stream);
int gs_frame_async_destroy(gs_frame_async *a);

/* Same work as gs_frame_forward, but brackets every stage with hipEvents on `stream` and
 * returns the stage durations in milliseconds (synchronises; for bench.py / profiling only):
 * stage_ms_host[0..5] = project+count, scan+emit, radix sort, tile ranges, raster, total. */
#define GS_N_STAGES 6
int gs_frame_forward_profile(const gs_frame *f, float *stage_ms_host, gs_stream_t stream);
/* Likewise for gs_frame_backward: [0..2] = raster backward (incl. memset + bucket scan),
 * project backward, total. */
int gs_frame_backward_profile(const gs_frame *f, const float *grad_image, float *grad_pos,
                              float *grad_quat, float *grad_scale, float *grad_opa,
                              float *grad_rgb, float *stage_ms_host, gs_stream_t stream);

/* Counters of the last forward on this workspace, copied device->host asynchronously into
 * `stats_host` (4 x int64: V visible, M pairs, overflow flag, processed buckets).  The
 * caller synchronises the stream before reading.  `processed buckets` (training frames; written by the backward's
 * preparation, i.e. it may still be the previous frame's when read right behind a forward): low 32 bits = buckets of 64
 * Gaussians in the backward's work list, high 32 bits = how many of them belong to saturated tiles (GS_FRAME_BWD_ROWS). */
int gs_frame_stats_async(const gs_frame *f, int64_t *stats_host, gs_stream_t stream);

/* Length of the longest tile list of the last forward on this workspace (sort_mode 2, strip variant; lists of up to
 * 1024 pairs are reported as 0), copied device->host asynchronously into *longest_host.  A caller that sees a value
 * above 2,048 sets GS_FRAME_LONG_SORT on the following frames; GS_FRAME_LONG_LISTS follows a cost model over the longest list,
 * the pairs and the pairs beyond 512 per tile (gs_frame.py, FrameRenderer._note_lists). */
int gs_frame_longest_list_async(const gs_frame *f, int64_t *longest_host, gs_stream_t stream);

/* The ABI-level guard against LAGGING counters (round 6).  A client that copies the counters
 * asynchronously and looks at them frames later -- to grow its workspace, to set GS_FRAME_LONG_SORT / GS_FRAME_LONG_LISTS /
 * GS_FRAME_BWD_ROWS -- must know WHICH frame they belong to: flags latched from the counters of frame k while frame k + 500
 * is being issued made a training run timing-dependent in round 5.  This call enqueues, on `stream`: a fill of the counter
 * block's tag word with `tag` (the client's frame number), then ONE device-to-host copy of GS_STATS_TAGGED_N = 15 values:
 *   [0] visible, [1] emitted pairs, [2] overflow (0, or the pairs the frame needed), [3] buckets (low 32 bits: in the
 *   backward's work list, high: of saturated tiles), [4..8] internal, [9] longest tile list (0 up to 1,024), [10] non-zero iff
 *   an occlusion-culled frame was rendered again from its full lists, [11] the tag (both 32-bit halves), [12] 0 (retired in ABI 8: the pairs beyond
 *   the first 512 of every list, summed with one atomic per long tile -- 14 us on the 2.4 M scene; see [14]), [13] the longest walk a tile's wave actually made in the compositing
 *   (0 up to 1,024; a tile whose pixels stop early walks less than its list), [14] the steps beyond the first 512 of every walk
 *   (what a GS_FRAME_LONG_LISTS frame would composite in segments; both from UNFLAGGED frames: a flagged frame's waves stop at 512).
 * stats_host[11] == tag (low half) <=> the copy has landed and the values are those of the frame issued just before this
 * call on `stream`.  stats_host should be pinned memory (the copy is asynchronous only then).  Recommended policy
 * (gs_frame.py): one copy in flight, and never issue frame k + 8 before the counters of frame k have been looked at. */
#define GS_STATS_TAGGED_N 15
int gs_frame_stats_tagged_async(const gs_frame *f, uint32_t tag, int64_t *stats_host, gs_stream_t stream);

/* Non-zero in *ran_past_host (after `stream` has reached this copy) iff the frame's lists had been trimmed
 * (GS_FRAME_OCCLUSION_CULL) and a tile ran past its cut, i.e. the frame was rendered a second time from the full lists.
 * On a GS_FRAME_CULL_REPEAT frame, which has no second pass, a non-zero value means: the caller's promise was broken, the
 * frame was NOT rendered again, and the image it delivered is not guaranteed to be the unculled frame.  (Zero means, as for
 * every culled frame, that the image is exact.)  The next forward of the workspace without that flag is repaired as usual. */
int gs_frame_cull_fallback_async(const gs_frame *f, int64_t *ran_past_host, gs_stream_t stream);

/* *enqueued = 1 iff a forward of this frame description enqueues the five gated launches of an occlusion-culled frame's second
 * pass: the frame is culled (gs_frame_is_occlusion_culled) and does not carry GS_FRAME_CULL_REPEAT.  Host-side, no launch, no
 * device.  GS_E_INVALID with the reason of the forward's refusal for GS_FRAME_CULL_REPEAT with GS_FRAME_CULL_DILATE. */
int gs_frame_cull_second_pass(const gs_frame *f, int32_t *enqueued);

/* *culled = 1 iff the library renders this frame description with the occlusion cull (the flag is set AND none of the
 * conditions under which it is ignored holds); host-side, no launch.  Such a frame's first pass tests every Gaussian
 * against the frustum and the cut pyramid on its position and scale alone and projects the survivors only: the rectangle
 * records (gs_frame_debug_rects) and the 64-byte records are then fresh for the PROJECTED Gaussians only -- the others keep
 * what an earlier frame left -- unless the frame fell back (second pass: everything is projected again). */
int gs_frame_is_occlusion_culled(const gs_frame *f, int32_t *culled);

/* (Validity, since ABI 4: `tiles_touched` is written by sort_modes 0 / 1 only -- sort_mode 2 keeps the count in
 * rects[i].w, gs_frame_debug_rects -- and the rec_* records are written for VISIBLE Gaussians only: the record of a
 * culled Gaussian holds whatever an earlier frame left there.  The culling mask is `rects[i].z != 0`, never
 * `rec_geom[i].z != 0`.)
 * Read-only views into the workspace of the last forward (for parity tests): sorted keys
 * (u64 [M]; NULL for a sort_mode-2 frame rendered without GS_FRAME_EMIT_SORTED_KEYS -- they are
 * (tile << 32 | depth bits of rec_geom[id].z) of the sorted ids), sorted Gaussian ids (u32 [M]), per-tile
 * ranges (int32 [T,2]), projected pos/cov/mask-equivalents.  Any out pointer may be NULL. */
int gs_frame_debug_views(const gs_frame *f, const uint64_t **sorted_keys,
                         const uint32_t **sorted_ids, const int32_t **tile_ranges,
                         const float **rec_geom, const float **rec_cov, const float **rec_color,
                         const uint32_t **tiles_touched);

/* Which binning / sort path gs_frame_forward takes for this frame description: 0 / 1 = sort_mode 0 / 1 (radix passes on
 * the 64-bit key / on its tile bits), 2 = sort_mode 2 with the table variant, 3 = slice-sorted variant, 4 = strip
 * variant (see GS_FRAME_STRIP_BIN for the size-based choice).  Negative: the description does not validate. */
int gs_frame_binning_variant(const gs_frame *f);

/* [N][4] uint32, written for EVERY Gaussian by every forward: (y0 | y1 << 16, x0 | x1 << 16, depth bits, tiles touched) --
 * the tile rectangle [y0, y1) x [x0, x1), the float bits of the depth |p_c|, the number of tiles listed.  The depth bits
 * are 0 exactly for the Gaussians the frustum test culled (the reference's culling_mask, renderer.py:123-132, is
 * `depth bits != 0`); the 64-byte record (rec_geom / rec_cov / rec_color above) of a culled Gaussian is NOT written and
 * holds whatever an earlier frame left there. */
int gs_frame_debug_rects(const gs_frame *f, const uint32_t **rects);

/* The per-tile occlusion cuts the last INFERENCE forward of this workspace left behind (uint32 [*n_tiles], row-major over the
 * tile grid): the float bits of the depth behind which the next GS_FRAME_OCCLUSION_CULL frame trims the tile's list, 0xffffffff
 * for a tile without a cut.  A read-only view, for tests: a GS_FRAME_CULL_REPEAT frame that kept its promise leaves the
 * table it read.  GS_E_INVALID for a training frame (training forwards do not write the table). */
int gs_frame_debug_cut_table(const gs_frame *f, const uint32_t **cut, int32_t *n_tiles);

/* The compact phase of the rgb inference compositing kernel (raster_fwd_body.h), per tile of the last forward of this workspace
 * (uint32 [*n_tiles], row-major over the tile grid): the number of Gaussians of its list the tile had composited when its wave
 * handed the live pixels over to the two-pixels-per-lane layout, 0xffffffff for a tile that never did (always, with
 * GS_FWD_COMPACT=0 in the environment, and in a GS_FRAME_LONG_LISTS frame).  A read-only view, for tests and measurements.
 * GS_E_INVALID unless the frame is an rgb inference frame without GS_FRAME_AUX (no other kernel writes the word). */
int gs_frame_debug_tile_compact(const gs_frame *f, const uint32_t **at, int32_t *n_tiles);

/* The Gaussians every tile composited before its wave stopped in the last forward of this workspace (uint32 [*n_tiles]): the
 * cost that orders the next forward's tiles.  Recorded by frames of the strip variant only (gs_frame_binning_variant == 4):
 * GS_E_INVALID for the others.  A read-only view, for tests and measurements. */
int gs_frame_debug_tile_cost(const gs_frame *f, const uint32_t **cost, int32_t *n_tiles);

/* Where the FIRST PASS of an occlusion-culled frame (gs_frame_is_occlusion_culled) stages its level-1 entries, for tests of
 * that path: slice s of the Gaussian array owns slots [s x *cap, (s + 1) x *cap) of *entries (8 bytes each) and *tags
 * (4 bytes each), both borrowed from the sort buffers of the workspace and overwritten by the rest of the frame, and wrote
 * (*slice_entries)[s] of them -- 0xffffffff: the slice had more than *cap entries, stored none beyond its slots and sent the
 * frame to its second pass.  Fails for a frame description that is not culled. */
int gs_frame_debug_cull_stage(const gs_frame *f, const uint64_t **entries, const uint32_t **tags,
                              const uint32_t **slice_entries, int32_t *slices, int64_t *cap);

/* [T] uint32: how many Gaussians of its list each tile's forward actually composited before all of its pixels had
 * stopped (a multiple of 64 except for the last chunk), kept by TRAINING forwards for the backward.  Measurement
 * aid: the compositing work of a frame is sum(tile_nproc) steps, not the pair count. */
int gs_frame_debug_tile_nproc(const gs_frame *f, const uint32_t **tile_nproc);

/* SH training frames whose raster backward ran on the matrix pipe (color_dim 27 / 48, frame path): [*n_slots] uint32, the
 * pixel-row steps (16 Gaussians x 16 pixels: 3 floor(NB / 4) + 12 fp32 MFMAs each) every wave of the LAST backward executed --
 * rows whose 16 pixels had all stopped are left out, so this, not 16 x the composited steps / 16, is what the kernel's
 * MFMA flops are counted from (bench.py).  *n_slots = 0 for frames that take another kernel.  Measurement aid. */
int gs_frame_debug_bwd_exec_rows(const gs_frame *f, const uint32_t **exec_rows, int32_t *n_slots);

/* Backward frame: grad_image is dL/d(image) [height,width,3] (w.r.t. the clamped, cropped
 * output).  Writes dL/d(raw parameter) for every Gaussian (zeros for culled ones):
 * grad_pos [N,3], grad_quat [N,4], grad_scale [N,3], grad_opa [N], grad_rgb [N,color_dim].
 * Must follow a gs_frame_forward with training=1 on the same workspace. */
int gs_frame_backward(const gs_frame *f, const float *grad_image, float *grad_pos,
                      float *grad_quat, float *grad_scale, float *grad_opa, float *grad_rgb,
                      gs_stream_t stream);

/* The same backward in three calls, for the view-parallel gradient exchange (gs_dp.py): GS_BWD_RASTER runs the raster
 * backward (per-pair gradient rows in the workspace; needs grad_image only), after which GS_BWD_GEOMETRY writes
 * grad_pos / grad_quat / grad_scale and GS_BWD_COLOR writes grad_opa / grad_rgb -- in either order, each bit-identical
 * to what gs_frame_backward writes -- so that the all-reduce of the bucket written first runs underneath the kernel
 * that writes the other one.  Pointers a part does not write may be NULL. */
#define GS_BWD_RASTER 1
#define GS_BWD_GEOMETRY 2
#define GS_BWD_COLOR 4
int gs_frame_backward_part(const gs_frame *f, const float *grad_image, float *grad_pos, float *grad_quat,
                           float *grad_scale, float *grad_opa, float *grad_rgb, int32_t part, gs_stream_t stream);

/* ABI 5 -- the frame in pieces, for the view-parallel trainer (gs_dp.py, gs_train.py; no reference analogue: the
 * reference is single-GPU).  The gradients of a frame only become final in the last kernel of the backward -- the
 * per-Gaussian sum of the per-pair gradient rows -- and that kernel is independent per Gaussian:
 *   gs_frame_backward_slice : after gs_frame_backward_part(GS_BWD_RASTER), the sums of the Gaussians [g_begin, g_end)
 *                             only (g_begin a multiple of 256; `part` = GS_BWD_GEOMETRY, GS_BWD_COLOR or both OR-ed:
 *                             both in ONE kernel, the rows are read once).  Any partition of [0, N) into ranges writes
 *                             exactly what gs_frame_backward writes, so that the exchange of one range's gradients
 *                             runs underneath the sums of the next.
 * and the NEXT frame's project stage (cull + project + activations + level-1 count) needs nothing but the parameters of
 * its own Gaussians:
 *   gs_frame_project_slices : *slices = how many slices of the Gaussian array the project stage of this frame is made
 *                             of (0: it cannot be issued in pieces -- only sort_mode 2's strip variant can),
 *                             *per_slice = Gaussians per slice (a multiple of 256);
 *   gs_frame_forward_project: the project stage of slices [slice_begin, slice_end) -- call it for every slice exactly
 *                             once, the range that starts at slice 0 first;
 *   gs_frame_forward_rest   : binning, per-tile sort, compositing.  project(all slices) + rest == gs_frame_forward.
 * Nothing of the previous frame's workspace contents that its backward still needs is touched by the project stage
 * except the per-Gaussian records and rectangles, i.e. issue a slice's project only after that slice's
 * gs_frame_backward_slice (same stream). */
int gs_frame_backward_slice(const gs_frame *f, float *grad_pos, float *grad_quat, float *grad_scale, float *grad_opa,
                            float *grad_rgb, int32_t part, int64_t g_begin, int64_t g_end, gs_stream_t stream);
int gs_frame_project_slices(const gs_frame *f, int32_t *slices, int64_t *per_slice);
int gs_frame_forward_project(const gs_frame *f, int32_t slice_begin, int32_t slice_end, gs_stream_t stream);
int gs_frame_forward_rest(const gs_frame *f, gs_stream_t stream);

/* ===================================================================================
 * Section C -- the training step around the frame
 * =================================================================================== */

/* torch.optim.Adam(betas=(beta1, beta2), eps) .step() of the reference trainer (train.py:59-67, :113;
 * no weight decay, no amsgrad) on ONE flat fp32 bucket: param / grad / exp_avg / exp_avg_sq [n], all
 * 16-byte aligned.  Parameter group k is the index range [group_end[k-1], group_end[k]) (group_end[-1] = 0,
 * group_end[n_groups-1] = n, n_groups <= 8) with learning rate lr[k]; both tables are HOST arrays.
 * `step` is the 1-based step count (bias corrections are evaluated in double on the host, like torch).
 * Optional densification statistic of train.py:145-154 for the index range [stat_begin, stat_end) (the
 * `pos` group): stat_mode 1: grad_stat = max(grad_stat, |grad|); 2: grad_stat += |grad|; 0: off. */
int gs_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                 int32_t n_groups, const int64_t *group_end, const float *lr, float beta1, float beta2,
                 float eps, int64_t step, float *grad_stat, int64_t stat_begin, int64_t stat_end,
                 int32_t stat_mode, gs_stream_t stream);

/* The same step restricted to the elements [range_begin, range_end) of the same arrays (group table and statistic range
 * stay absolute): one bucket of the view-parallel gradient exchange at a time, so that the update of the bucket whose
 * all-reduce has finished runs underneath the all-reduce of the next one.  Every element's update is what gs_adam_step
 * computes for it.  The statistic is only touched where its range intersects [range_begin, range_end). */
int gs_adam_step_range(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                       int64_t range_begin, int64_t range_end, int32_t n_groups, const int64_t *group_end,
                       const float *lr, float beta1, float beta2, float eps, int64_t step, float *grad_stat,
                       int64_t stat_begin, int64_t stat_end, int32_t stat_mode, gs_stream_t stream);

/* View-parallel training with a SHARDED optimizer (reduce-scatter -> this step -> all-gather of the parameters): the
 * rank owns elements [range_begin, range_end) of the flat index space and keeps only THEIR moments: exp_avg_shard[0] /
 * exp_avg_sq_shard[0] belong to element `moment_base` (a multiple of 4, <= range_begin); param / grad / the group table
 * and the statistic range stay absolute.  `skip_if_nonzero` (may be NULL) is the device address of a 64-bit counter:
 * when it is non-zero the launch leaves everything untouched -- pass gs_frame_overflow_flag() so that a training frame
 * that overflowed its workspace (rendered empty, all-zero gradient) does not move the parameters by momentum, without
 * any host synchronisation.  Every element's update is what gs_adam_step computes for it. */
int gs_adam_step_sharded(float *param, const float *grad, float *exp_avg_shard, float *exp_avg_sq_shard, int64_t n,
                         int64_t range_begin, int64_t range_end, int64_t moment_base, int32_t n_groups,
                         const int64_t *group_end, const float *lr, float beta1, float beta2, float eps, int64_t step,
                         float *grad_stat, int64_t stat_begin, int64_t stat_end, int32_t stat_mode,
                         const void *skip_if_nonzero, gs_stream_t stream);

/* Up to 8 element ranges [range_begin[r], range_end[r]) of the same flat arrays in ONE launch (host tables;
 * range_begin a multiple of 4): one slice of the view-parallel exchange is a range of Gaussians in each of the five
 * parameter arrays.  The moments of range r start at exp_avg + moment_offset[r] (a multiple of 4): element i keeps its
 * moments at index moment_offset[r] + (i - range_begin[r]) -- moment_offset = range_begin for a replicated optimizer,
 * densely packed shards for a sharded one.  Group table, statistic and skip flag as in gs_adam_step_sharded.
 * grad_scale: the gradient enters as grad * grad_scale -- 1 / world when the exchange SUMS the ranks' gradients and
 * leaves the mean to the optimizer (RCCL's ReduceOp.AVG is a pre-multiplied sum that launches a scaling kernel even on
 * one rank; SUM does not), 1 otherwise: every element's update is then what gs_adam_step computes for it. */
int gs_adam_step_multi(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t n_ranges,
                       const int64_t *range_begin, const int64_t *range_end, const int64_t *moment_offset,
                       int32_t n_groups, const int64_t *group_end, const float *lr, float beta1, float beta2, float eps,
                       int64_t step, float *grad_stat, int64_t stat_begin, int64_t stat_end, int32_t stat_mode,
                       const void *skip_if_nonzero, float grad_scale, gs_stream_t stream);

/* Single-GPU training step (round 5: rgb colours; round 6: SH colours too): gs_frame_backward whose LAST kernel -- the per-Gaussian sum of the gradient
 * rows + projection / activation backward -- applies the Adam update to the Gaussian's 14 parameters on the spot instead of
 * writing their gradients.  The gradient never travels through memory (2 x 56 B per Gaussian) and the optimizer's stream of
 * parameters and moments runs underneath the projection backward's arithmetic (that kernel is VALU-bound, gs_adam_step
 * HBM-bound).  Every updated value is bit for bit what gs_frame_backward + gs_adam_step give (same expressions, same
 * rounding); culled Gaussians take their zero-gradient step (momentum) as they do there.
 *   The PARAMETERS updated in place are the frame's own f->pos, quat, scale, opa, rgb (the descriptor calls them const: they
 * are not, here); exp_avg / exp_avg_sq: their moments, same shapes, in the order pos, quat, scale, opa, rgb; lr likewise;
 * step counts from 1; grad_stat (may be NULL with stat_mode 0): [N,3], max (1) or sum (2) of |dL/dpos| folded in
 * (train.py:145-154); skip_if_nonzero (may be NULL): device address of a 64-bit counter -- non-zero: the step is skipped (the
 * frame's overflow counter, gs_frame_overflow_flag).  SH frames (color_dim 27 / 48): the wave that sums a Gaussian's
 * coefficient gradients steps the coefficients where it would have stored the gradients (+1 % on the SH training step: the
 * coefficient gradients' round trip and one launch; the optimizer's own stream stays).  No gradient buffer is written. */
typedef struct gs_adam_fused {
    float *exp_avg[5], *exp_avg_sq[5];
    float lr[5];
    float beta1, beta2, eps;
    int64_t step;
    float *grad_stat;
    int32_t stat_mode;
    const void *skip_if_nonzero;
} gs_adam_fused;
int gs_frame_backward_adam(const gs_frame *f, const float *grad_image, const gs_adam_fused *adam, gs_stream_t stream);

/* The same step for GS_FRAME_AUX training frames (RGB-D training: colour and depth supervision in one step).  The raster
 * backward takes f->grad_depth / f->grad_alpha (NULL = zero) next to grad_image, which may be NULL here (zero: a depth-only
 * step; the library then reads a zero image of its own, allocated once per device at the first such call), and the
 * projection backward adds the depth map's position term rot^T (g_d p_c / |p_c|) -- g_d = the sum of the Gaussian's depth
 * floats over the same rows in the same ascending order as frame_aux_depth_backward_kernel takes them -- to dL/dpos before it
 * steps.  Every updated parameter, both moments and the grad_stat fold are bit for bit what gs_frame_backward of the
 * flagged frame + gs_adam_step give; culled Gaussians take their zero-gradient step, skip_if_nonzero skips the step of an
 * overflowed frame.  GS_E_INVALID for a frame without GS_FRAME_AUX (gs_frame_backward_adam is its entry point), a frame
 * that is not a training frame, a NULL or invalid `adam`; GS_E_UNSUPPORTED with GS_FRAME_POSE_GRAD.  Everything is checked
 * before anything is enqueued.  rgb and SH colours (color_dim 3 / 27 / 48). */
int gs_frame_backward_adam_aux(const gs_frame *f, const float *grad_image, const gs_adam_fused *adam, gs_stream_t stream);

/* The same step for GS_FRAME_POSE_GRAD training frames, with or without GS_FRAME_AUX (joint refinement of a keyframe's pose
 * and the map): the raster backward, ONE kernel that sums the rows, forms every Gaussian's pose terms from the position,
 * quaternion and scale it loaded before the step, sums them per workgroup and steps the 14 parameters, and the reduction of
 * the partial rows into f->grad_rot / f->grad_tran.  The pose gradient belongs to the parameters the frame was rendered
 * with.  Every updated parameter, both moments and the grad_stat fold are bit for bit what gs_frame_backward of the flagged
 * frame + gs_adam_step give, and grad_rot / grad_tran are bit for bit what that gs_frame_backward writes (the same partial
 * rows in the same layout: one per workgroup of 256 Gaussians, with GS_FRAME_AUX a second one for the depth map's term).
 * With GS_FRAME_AUX the call reads f->grad_depth / f->grad_alpha and grad_image may be NULL, as in
 * gs_frame_backward_adam_aux.  An overflowed frame takes no step (skip_if_nonzero) and gets zero pose gradients; N = 0
 * writes zero pose gradients.  GS_E_INVALID for a frame without GS_FRAME_POSE_GRAD, a frame that is not a training frame, a
 * NULL or invalid `adam`; GS_E_UNSUPPORTED with SH colours (color_dim 27 / 48: the image also depends on the pose through
 * the pixels' ray directions).  Everything is checked before anything is enqueued. */
int gs_frame_backward_adam_pose(const gs_frame *f, const float *grad_image, const gs_adam_fused *adam, gs_stream_t stream);

/* The pose gradient of a GS_FRAME_POSE_GRAD training frame (rgb colours; with or without GS_FRAME_AUX) and nothing else, for a
 * caller that holds the map fixed (camera tracking): no per-Gaussian gradient is computed, stored or given a destination.
 *   part 0               : the raster backward -- the stage gs_frame_backward_part(GS_BWD_RASTER) runs, with GS_FRAME_AUX
 *                          reading f->grad_depth / f->grad_alpha as they are; grad_image must not be NULL --, then ONE kernel
 *                          that sums every Gaussian's rows, forms its pose terms (with GS_FRAME_AUX the depth map's as well)
 *                          and leaves the partial rows, then their reduction into f->grad_rot / f->grad_tran;
 *   part GS_BWD_GEOMETRY : that kernel and the reduction, from the rows a preceding gs_frame_backward_part(GS_BWD_RASTER) of
 *                          the same frame left; grad_image is not read.
 * f->grad_rot / f->grad_tran and every partial row of the pose workspace are bit for bit what
 * gs_frame_backward_part(GS_BWD_GEOMETRY) -- and so gs_frame_backward and gs_frame_backward_adam_pose -- leave for the same
 * frame.  N = 0 and an overflowed frame get zeros.  Refusals, all before anything is enqueued, the first that applies: an
 * invalid descriptor (the pose fields included); GS_E_INVALID for a frame that is not a training frame, a `part` other than 0
 * or GS_BWD_GEOMETRY, a frame without GS_FRAME_POSE_GRAD; GS_E_UNSUPPORTED with SH colours; GS_E_INVALID for a NULL
 * grad_image with part 0. */
int gs_frame_backward_pose(const gs_frame *f, const float *grad_image, int32_t part, gs_stream_t stream);

/* Device address of the frame's overflow counter (inside the caller's workspace; 64-bit, 0 = the last forward of this
 * frame description fitted its pair capacity, else the pair count it would have needed).  No launch, no copy. */
int gs_frame_overflow_flag(const gs_frame *f, const void **device_counter);

/* The same statistic without the Adam update: stat[i] = max(stat[i], |grad[i]|) (stat_mode 1) or stat[i] += |grad[i]|
 * (stat_mode 2) for i < n.  View-parallel training (one view per GPU) needs it: train.py:145-154 accumulates the
 * |gradient| of EACH VIEW, so every rank updates the statistic from its own gradient before the all-reduce averages
 * the gradients, and the statistics are combined (max / sum over ranks) at the densification boundaries. */
int gs_grad_stat_update(const float *grad, float *stat, int64_t n, int32_t stat_mode, gs_stream_t stream);

/* Image loss of train.py:99-107 and its gradient:
 *   loss = (1 - ssim_weight) * mean|pred - target| + ssim_weight * (1 - SSIM(pred, target)),
 * SSIM = torchmetrics StructuralSimilarityIndexMeasure(data_range=1.0) (11x11 Gaussian window, sigma 1.5,
 * evaluated on the pixels whose window lies inside the image).  pred, target, grad: [H, W, 3] fp32;
 * grad = dloss/dpred.  loss_out (device, may be NULL) receives (loss, l1 mean, ssim mean).
 * ssim_weight = 0 skips the SSIM passes (any image size); otherwise H, W must exceed 10. */
size_t gs_loss_workspace_bytes(int32_t H, int32_t W);
int gs_loss_l1_ssim(const float *pred, const float *target, int32_t H, int32_t W, float ssim_weight,
                    float *grad, float *loss_out, void *workspace, size_t workspace_bytes,
                    gs_stream_t stream);

/* gs_loss_l1_ssim with a per-pixel weight map `weight` [H, W] fp32 (finite and >= 0 -- NOT checked here: the caller validates
 * a map once; the three channels of a pixel share its weight).  With m the weight of a pixel and S the SSIM map on the
 * interior (rows 5 .. H - 6, columns 5 .. W - 6):
 *   l1   = sum_p m_p sum_c |x - y|        / (3 weight_sum)
 *   ssim = sum_{q interior} m_q sum_c S_qc / (3 weight_sum_interior)
 *   loss = (1 - w) l1 + w (1 - ssim)
 *   dL/dx = a m sign(x - y) - b [ g*(m D_mu) + 2 x g*(m D_xx) + y g*(m D_xy) ],
 *   a = (float)((1 - w) / (3 weight_sum)),  b = (float)(w / (3 weight_sum_interior)).
 * weight_sum and weight_sum_interior -- the sum of the map and its sum over the interior -- are HOST arguments: the caller
 * takes them once per view; there is no count pass and no host synchronisation.  weight_sum == 0: the L1 term, its value and
 * its gradient are exactly 0.  weight_sum_interior == 0 or w == 0: the SSIM term (in loss_out[0] too), loss_out[2] and its
 * gradient are exactly 0, and the weighted L1 kernel runs alone (any image size when w == 0).  A pixel of weight 0 takes no
 * part in the SSIM term at all: its S is not read, its adjoints are +0.0f, so its gradient is exactly +0.0f where no
 * interior pixel of non-zero weight lies within 5 rows and 5 columns.  An all-ones map with weight_sum = H W and
 * weight_sum_interior = (H - 10)(W - 10) gives gs_loss_l1_ssim's gradient and values bit for bit.  loss_out = (loss, l1,
 * ssim) as there; the workspace is gs_loss_workspace_bytes(H, W).
 * GS_E_INVALID -- before anything is enqueued, the first that applies --: H or W <= 0; a NULL pred, target, weight or grad;
 * ssim_weight outside [0, 1] or NaN; ssim_weight > 0 with H <= 10 or W <= 10; a sum that is negative, infinite or NaN; a
 * workspace that is NULL or too small. */
int gs_loss_l1_ssim_weighted(const float *pred, const float *target, const float *weight, int32_t H, int32_t W,
                             float ssim_weight, double weight_sum, double weight_sum_interior, float *grad, float *loss_out,
                             void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* Depth supervision on the maps of a GS_FRAME_AUX frame: depth D = sum_i w_i d_i and alpha A = sum_i w_i, [H,W] fp32, against
 * a measured RANGE `target` [H,W] (distance from the camera centre, as d_i = |p_c| is; z-depth is converted by the caller:
 * range = z |ray| / ray_z).  A target pixel that is <= 0, infinite or NaN carries no measurement and does not count.
 *   mode 0: r = D - A target  (= sum_i w_i (d_i - target): no division, defined everywhere)
 *   mode 1: r = D / A - target  (the expected depth), counted only where A >= alpha_min (> 0)
 *   loss = scale * sum_counted |r|,  grad_depth = scale sign(r) dr/dD,  grad_alpha = scale sign(r) dr/dA,
 * both gradients exactly zero where the pixel does not count.  Put weight / (number of valid target pixels) into `scale`:
 * no count pass, no host synchronisation.  loss_out (device, may be NULL) receives (loss, number of pixels that counted --
 * exact up to 2^24).  The five maps must be 16-byte aligned.  One streaming pass and a one-workgroup reduction in double,
 * fixed order, no atomics: bitwise repeatable.  The two gradient maps are what gs_frame.grad_depth / grad_alpha take. */
size_t gs_loss_depth_workspace_bytes(int32_t H, int32_t W);
int gs_loss_depth(const float *depth, const float *alpha, const float *target, int32_t H, int32_t W, int32_t mode,
                  float alpha_min, float scale, float *grad_depth, float *grad_alpha, float *loss_out, void *workspace,
                  size_t workspace_bytes, gs_stream_t stream);

/* The loss of camera tracking against a frozen map, on a GS_FRAME_AUX frame rendered from the pose under estimation: image
 * [H,W,3], depth D [H,W] and alpha A [H,W] against the incoming frame's target_image [H,W,3] and target_range [H,W] (NULL:
 * RGB-only tracking; a pixel that is <= 0, infinite or NaN carries no measurement -- the rule of gs_loss_depth).  Per pixel, in
 * fp32 with one rounding per operation, cs = fl(scale color_weight), ds = fl(scale depth_weight):
 *   colour: counts iff A >= alpha_min (> 0: the silhouette of the map);  term = cs sum_c |I_c - T_c|,
 *           grad_image_c = +cs / -cs by the sign of I_c - T_c, 0 where they are equal;
 *   depth : counts iff the pixel counts for colour, carries a measurement z and, with r = D / A - z, depth_gate <= 0 (off)
 *           or |r| <= depth_gate;  term = ds |r|,  grad_depth = s (1 / A),  grad_alpha = -s ((D / A) / A),  s = +ds / -ds
 *           by the sign of r (gs_loss_depth mode 1, bit for bit where ds equals its scale);
 * every other gradient is written as an exact zero; the masks are constants and are not differentiated.  values_out (device,
 * 4-byte aligned, may be NULL) receives (loss = colour term + depth term, colour term, depth term, pixels that counted for
 * depth -- exact up to 2^24).  The caller picks `scale` (finite; 1 / (H W) makes the terms means over the image): no count
 * pass, no host synchronisation.  The eight maps must be 16-byte aligned, the workspace too.  One streaming pass (four
 * consecutive pixels per lane) and a one-workgroup reduction in double, fixed order, no atomics: bitwise repeatable.
 * GS_E_INVALID -- before anything is enqueued -- for a null pointer, H or W <= 0, a misaligned map, alpha_min <= 0 or NaN, a
 * negative or NaN weight, a scale that is not finite, a workspace that is null, misaligned or too small.  The three gradient
 * maps are what gs_frame_backward takes as grad_image and gs_frame.grad_depth / grad_alpha. */
size_t gs_loss_track_workspace_bytes(int32_t H, int32_t W);
int gs_loss_track(const float *image, const float *depth, const float *alpha, const float *target_image,
                  const float *target_range, int32_t H, int32_t W, float alpha_min, float color_weight, float depth_weight,
                  float depth_gate, float scale, float *grad_image, float *grad_depth, float *grad_alpha, float *values_out,
                  void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* gs_loss_track with a median gate in place of the fixed depth_gate: a term counts where its residual is at most k x the
 * LOWER MEDIAN of that residual over the frame (SplaTAM's outlier rule), decided on the device.  Every argument of
 * gs_loss_track except depth_gate, with its meaning; per pixel, in fp32 with one rounding per operation and the expressions
 * of gs_loss_track in their order:
 *   covered = A >= alpha_min,   c = (|d_0| + |d_1|) + |d_2| with d = I - T,   e = D / A,  r = e - z,  a = |r|.
 *   S_d = covered, measured (the rule of gs_loss_depth) and a <= FLT_MAX (false for NaN);  S_c = covered and c <= FLT_MAX;
 *   n_d = |S_d|, n_c = |S_c|;  m_d = the element of rank floor((n_d - 1) / 2) of S_d's a values in ascending order -- an
 *   element of the set, never an average --, 0 for an empty set;  m_c likewise over c.  Both are taken before any gating.
 *   t_d = max(fl(depth_gate_k m_d), depth_gate_floor),   t_c = max(fl(color_gate_k m_c), color_gate_floor).
 *   depth  counts iff covered, measured and (depth_gate_k <= 0 or (a <= FLT_MAX and a <= t_d));
 *   with couple != 0 and depth_gate_k > 0 a pixel of S_d that fails its depth gate loses its colour term too (an occluder
 *   has the wrong colour as well);
 *   colour counts iff covered, not dropped by the coupling, and (color_gate_k <= 0 or (c <= FLT_MAX and c <= t_c)).
 * Where a term counts its gradients are, bit for bit, those gs_loss_track writes with depth_gate <= 0 and the same scale and
 * weights; everywhere else they are exact zeros.  With both k <= 0 the gradients and values_out[0..3] are gs_loss_track's.
 * values_out (device, 4-byte aligned, 8 floats, may be NULL) receives (loss, colour term, depth term, depth pixels that
 * counted, colour pixels that counted, m_d, m_c, n_d), the sums in gs_loss_track's fixed order in double.  resid_depth /
 * resid_color ([H,W], 16-byte aligned, each may be NULL: the map then lives in the workspace) receive a and c at the pixels
 * of S_d / S_c and a NaN at every other pixel.  Launches: one memset of the select's counters, a residual pass (reads the
 * five inputs once, writes a and c), two digit passes over a and c, the gated loss pass, the one-workgroup sum -- see
 * csrc/track_gate.hip.  No host synchronisation (the thresholds never leave the device), integer counting only, no float
 * atomics: bitwise repeatable.
 * GS_E_INVALID -- before anything is enqueued -- for everything gs_loss_track refuses, a NaN or negative floor, a NaN k, a
 * misaligned residual map, and H W > 2^24 (the counts are returned as floats and must be exact). */
size_t gs_loss_track_gated_workspace_bytes(int32_t H, int32_t W);
int gs_loss_track_gated(const float *image, const float *depth, const float *alpha, const float *target_image,
                        const float *target_range, int32_t H, int32_t W, float alpha_min, float color_weight,
                        float depth_weight, float depth_gate_k, float color_gate_k, float depth_gate_floor,
                        float color_gate_floor, int32_t couple, float scale, float *grad_image, float *grad_depth,
                        float *grad_alpha, float *values_out, float *resid_depth, float *resid_color, void *workspace,
                        size_t workspace_bytes, gs_stream_t stream);

/* The gate of gs_loss_track_gated as the MAPPING INPUTS of a keyframe: a GS_FRAME_AUX frame of the frozen map rendered at the
 * frame's pose (image, depth, alpha) and the incoming frame (target_image, target_range) give a range map without the
 * measurements the depth gate rejects and a per-pixel colour weight.  covered, measured, the residuals a and c, the sets S_d /
 * S_c, the lower medians m_d / m_c, the thresholds t_d / t_c and the two decisions "the depth term counts" (dmask) and "the
 * colour term counts" (cmask, the coupling included) are those of gs_loss_track_gated, unchanged.  Per pixel:
 *   range_out  = target_range where the pixel is measured and not (covered and measured and not dmask); else exactly +0.0f
 *                (an unmeasured input -- <= 0, inf, NaN -- is written as +0.0f too);
 *   weight_out = 0.0f where covered and not cmask, else 1.0f.
 * A pixel the map does not cover keeps its range and has weight 1: it is new surface, what seeding and mapping are for.  With
 * both k <= 0 nothing is gated: range_out is the measured input, weight_out all ones.  target_range may be NULL (an RGB-only
 * gate); range_out must then be NULL too, and only then.  values_out (device, 4-byte aligned, 8 floats, may be NULL) receives
 * (measured pixels, range pixels kept, range pixels removed, sum of weight_out, sum of weight_out over the SSIM interior --
 * rows 5 .. H - 6, columns 5 .. W - 6; 0 when H <= 10 or W <= 10 --, m_d, m_c, n_d); the counts are exact integers.
 * resid_depth / resid_color as in gs_loss_track_gated.  Launches: gs_loss_track_gated's memset, residual pass and two digit
 * passes as they are, one mask pass in place of the loss pass (reads alpha, the range and the two residual maps), a
 * one-workgroup sum of the workgroups' integer counts.  No float atomics, no host synchronisation: bitwise repeatable.
 * GS_E_INVALID -- before anything is enqueued, the first that applies --: H or W <= 0; H W > 2^24; a NULL image, depth, alpha,
 * target_image or weight_out; target_range and range_out not both NULL or both given; alpha_min <= 0 or NaN; a NaN k; a NaN
 * or negative floor; a map (inputs, outputs, residual maps) that is not 16-byte aligned; a values_out that is not 4-byte
 * aligned; an output (range_out, weight_out, values_out, resid_depth, resid_color) that overlaps an input or another
 * output; a workspace that is null, misaligned or smaller than gs_track_gate_mask_workspace_bytes(H, W). */
size_t gs_track_gate_mask_workspace_bytes(int32_t H, int32_t W);
int gs_track_gate_mask(const float *image, const float *depth, const float *alpha, const float *target_image,
                       const float *target_range, int32_t H, int32_t W, float alpha_min, float depth_gate_k,
                       float color_gate_k, float depth_gate_floor, float color_gate_floor, int32_t couple, float *range_out,
                       float *weight_out, float *values_out, float *resid_depth, float *resid_color, void *workspace,
                       size_t workspace_bytes, gs_stream_t stream);

/* One level down of an image pyramid: the targets of coarse-to-fine camera tracking (csrc/pyramid.hip).  image [H,W,3] and
 * range [H,W] (NULL: RGB only; range_out must then be NULL too) give image_out [H/2,W/2,3] and range_out [H/2,W/2]; H and W
 * are even.  Coarse pixel (i, j) covers the fine pixels (2i..2i+1, 2j..2j+1), named 00, 01, 10, 11 in row-major order.  Per
 * coarse pixel, in fp32 with one rounding per operation:
 *   colour, per channel: fl(fl(fl(fl(a00 + a01) + a10) + a11) 0.25f).  There is no rule for NaN: it propagates.
 *   range : a fine pixel is measured iff it is > 0 and finite (the rule of gs_loss_depth and gs_loss_track).  n = the number of
 *           measured pixels among the four, lo / hi = the minimum / maximum over them.  The coarse pixel is measured iff
 *           n >= min_valid and (edge_rel < 0 or hi <= fl(fl(1 + edge_rel) lo)); its value is fl(s / (float)n) with
 *           s = fl(fl(fl(v00 + v01) + v10) + v11), v = the range where measured and +0.0f where not.  An unmeasured coarse
 *           pixel is written as exactly 0.0f.
 * The edge test exists because a footprint that straddles a depth discontinuity has no range worth tracking against: dropping
 * it is the conservative choice.  A coarse pixel's ray passes through the corner its four fine pixels share; the mean of four
 * ranges along four slightly different rays is a SECOND-ORDER APPROXIMATION of the range along that ray: these targets are
 * for tracking, not for seeding or mapping.  Level l of a pyramid is this call applied l times (at most
 * GS_PYRAMID_MAX_LEVELS in gs_pyramid.Pyramid); there is no multi-level entry point.  The camera of level l: width, height,
 * focal lengths and the principal point in pixels (pixel (i, j) covers [i, i+1) x [j, j+1)) all divided by 2^l -- exact.
 * One launch: a lane makes four consecutive coarse pixels of one row, 256 lanes per workgroup, one item per lane (no grid
 * cap); 16-byte accesses when W % 8 == 0, else 4-byte accesses.  No atomics: bitwise repeatable.  No host synchronisation.
 * GS_E_INVALID -- before anything is enqueued -- for a NULL image, image_out or opts; range and range_out not both NULL or
 * both given; H or W <= 0 or odd; any pointer not 16-byte aligned; min_valid outside 1..4; a NaN edge_rel; an output that
 * overlaps an input; an image of 2^31 or more groups of four coarse pixels. */
#define GS_PYRAMID_MAX_LEVELS 4
typedef struct gs_pyramid_opts {
    int32_t min_valid; /* 1..4: a coarse range pixel needs this many measured fine pixels */
    float edge_rel;    /* < 0: off; else a footprint counts only where hi <= (1 + edge_rel) lo */
} gs_pyramid_opts;
int gs_pyramid_down(const float *image, const float *range, int32_t H, int32_t W, const gs_pyramid_opts *opts,
                    float *image_out, float *range_out, gs_stream_t stream);

/* ---- densification: Gaussian3ds.adaptive_control (splatter.py:122-228) ----
 * Two calls because the number of split Gaussians decides how many standard-normal draws the split
 * samples consume (the reference's MultivariateNormal.sample() draws them after its masks are known):
 *   gs_densify_classify: classes + counts_dev[4] = (kept, cloned, split, kept + cloned + split);
 *   gs_densify_apply   : writes the new Gaussian set in the reference's order -- kept ones (split ones
 *                        with scale / 1.6 (abs) or - log 1.6 (exp) and the first sample), clones
 *                        (pos - grad * clone_dt), second split samples.  eps1 / eps2: [n_eps, 3]
 *                        standard normals, n_eps >= split count; outputs hold `capacity` Gaussians.
 *                        Nothing is written if the total exceeds `capacity` or the split count n_eps.
 * A sample is pos + chol(R S^2 R^T) eps (utils.py:391-402).  grad: [N, 3] accumulated |grad_pos| statistic
 * (train.py:160).  All arrays fp32, rgb [N, color_dim]; the same workspace must be passed to both calls. */
typedef struct gs_densify_opts {
    float taus;              /* --split_thresh: ||act(scale)|| above which a Gaussian is split, else cloned */
    float delete_thresh;     /* --delete_thresh: Gaussians with ||act(scale)|| >= this are pruned            */
    float grad_thresh;       /* --grad_thresh                                                                 */
    float clone_dt;          /* --clone_dt                                                                    */
    int32_t scale_activation;/* 0 = abs, 1 = exp                                                              */
    int32_t grad_aggregation;/* 0 = max over xyz, 1 = mean                                                    */
    int32_t use_clone, use_split;
    int32_t color_dim;       /* 3, 27 or 48 (the colour row is copied through)                                */
} gs_densify_opts;
size_t gs_densify_workspace_bytes(int64_t N);
int gs_densify_classify(const float *scale, const float *opa, const float *grad, int64_t N,
                        const gs_densify_opts *opts, int64_t *counts_dev, void *workspace,
                        size_t workspace_bytes, gs_stream_t stream);
int gs_densify_apply(const float *pos, const float *quat, const float *scale, const float *opa,
                     const float *rgb, const float *grad, int64_t N, const gs_densify_opts *opts,
                     const float *eps1, const float *eps2, int64_t n_eps, float *out_pos, float *out_quat,
                     float *out_scale, float *out_opa, float *out_rgb, int64_t capacity,
                     const int64_t *counts_dev, void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- seeding from an RGB-D frame: new Gaussians where a depth camera saw a surface the model does not explain ----
 * Two calls around one host read, because the caller sizes the parameter arrays between them (as gs_densify_*):
 *   gs_seed_classify: decides every LATTICE pixel -- (x, y) with x % stride == stride / 2 and y % stride == stride / 2 -- and
 *                     writes counts_dev[2] = (selected, lattice pixels that carry a measurement);
 *   gs_seed_apply   : writes the selected pixels' Gaussians as rows [offset, offset + selected) of pos [.,3], quat [.,4],
 *                     scale [.,3], opa [.], rgb [., color_dim], arrays of `capacity` rows, in row-major pixel order.  Nothing
 *                     is written if offset + selected > capacity (counts_dev still holds the need).
 * range [H,W]: the measured distance from the camera centre (what the GS_FRAME_AUX depth map accumulates; z-depth is
 * converted by the caller), "no measurement" where it is <= 0, infinite or NaN -- the rule of gs_loss_depth.  image [H,W,3]:
 * fp32 in [0,1].  depth = sum_i w_i d_i and alpha = sum_i w_i [H,W]: the current model's maps from that camera, both or
 * neither; NULL: an empty model, every measured lattice pixel is selected.  The decision, in fp32 with one rounding per
 * operation (a float32 restatement decides identically):
 *   selected  <=>  measured  and  (no maps  or  A < alpha_thresh  or  z * A < (1 - front_rel) * D)
 * -- the last: the measurement lies in front of the expected depth D / A by more than the relative margin, without a division.
 * A selected pixel becomes the Gaussian
 *   pos   = rot^T (p_c - tran),  p_c = z_cam (u, v, 1),  z_cam = z / sqrt(u u + v v + 1),  (u, v) the renderer's own ray through
 *           the pixel centre: u = (x + left - padW / 2 + 0.5) / focal_x with the padded size and centred crop of the frame
 *           path (likewise v), so the Gaussian projects back onto the centre of its pixel;
 *   quat  = (1, 0, 0, 0);
 *   scale = isotropic, activated value sigma = scale_factor * stride * z_cam / ((focal_x + focal_y) / 2), stored as the
 *           inverse of the frame path's activation: max(sigma - 1e-4, 0) for abs (|s| + 1e-4), log(sigma) for exp;
 *   opa   = logit(opa_init);
 *   rgb   = logit(c) per channel, c clamped to [1 / 512, 1 - 1 / 512] (half an 8-bit step: |logit| <= 6.24); color_dim 27 /
 *           48: that logit / 0.28209479177387814 in the DC coefficient of each channel (channel-major 3 x 9 / 3 x 16, as
 *           utils.py:345-348), every other coefficient 0.
 * With opa_init > alpha_thresh a pixel that was seeded is not selected again from the same view: its own Gaussian gives it
 * A >= opa_init at its centre.  Ranks come from wave ballots, per-workgroup counts and a scan -- no atomics: the output is a
 * pure function of the inputs, bitwise repeatable.  The same workspace and opts go to both calls; quat must be 16-byte
 * aligned.  Everything is validated before anything is enqueued; all launches on `stream`. */
typedef struct gs_seed_opts {
    int32_t stride;           /* >= 1: lattice step in pixels                                                   */
    float alpha_thresh;       /* a pixel with rendered alpha below this is unexplained                          */
    float front_rel;          /* ... or one measured in front of the expected depth by more than this share     */
    float scale_factor;       /* sigma in lattice steps at the point's depth                                    */
    float opa_init;           /* in (0, 1)                                                                      */
    int32_t scale_activation; /* 0 = abs, 1 = exp                                                               */
    int32_t color_dim;        /* 3, 27 or 48                                                                    */
} gs_seed_opts;
typedef struct gs_seed_camera { /* as gs_frame carries it */
    float rot[9], tran[3];    /* world -> camera: p_c = rot p + tran (row-major)                                */
    float focal_x, focal_y;
    int32_t width, height;
} gs_seed_camera;
size_t gs_seed_workspace_bytes(int32_t H, int32_t W);
int gs_seed_classify(const float *range, const float *depth, const float *alpha, int32_t H, int32_t W,
                     const gs_seed_opts *opts, int64_t *counts_dev, void *workspace, size_t workspace_bytes,
                     gs_stream_t stream);
int gs_seed_apply(const float *image, const float *range, const gs_seed_camera *cam, const gs_seed_opts *opts, float *pos,
                  float *quat, float *scale, float *opa, float *rgb, int64_t offset, int64_t capacity,
                  const int64_t *counts_dev, const void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* A camera whose principal point is off the renderer's centre (GS_FRAME_PRINCIPAL_POINT: pp_dx = cx - cx0, pp_dy = cy - cy0 in
 * pixels).  gs_seed_apply_pp is gs_seed_apply with the ray of pixel (x, y) moved accordingly, in fp32, one rounding per
 * operation:
 *   u = fl(fl(fl((float)(x + left - padW / 2) + 0.5f) - pp_dx) / focal_x),  v likewise
 * -- the seeded Gaussian projects onto the centre of its pixel in a frame of the same camera.  Everything else, the workspace
 * and gs_seed_classify (which sees no camera) are as above.  Refuses an offset that is not finite.  gs_seed_camera and
 * gs_seed_apply keep their layout, signature and device code. */
typedef struct gs_seed_camera_pp {
    gs_seed_camera cam;
    float pp_dx, pp_dy;
} gs_seed_camera_pp;
int gs_seed_apply_pp(const float *image, const float *range, const gs_seed_camera_pp *cam, const gs_seed_opts *opts, float *pos,
                     float *quat, float *scale, float *opa, float *rgb, int64_t offset, int64_t capacity,
                     const int64_t *counts_dev, const void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- covisibility: of the surface points a frame measured, how many does each keyframe see? ----
 * range [H,W] (H, W = cam->height, cam->width): the incoming frame's measured range, "no measurement" where it is <= 0,
 * infinite or NaN (the rule of gs_seed and gs_loss_depth).  cam: the frame's posed camera, by value, on the host.
 * views_dev: a DEVICE array of n_views gs_seed_camera rows, 64 bytes = one line per view, 64-byte aligned; the caller keeps
 * one table and appends a row per keyframe.  counts_dev [n_views + 2] int64 on the device:
 *   [k]           measured lattice pixels whose point view k sees
 *   [n_views]     measured lattice pixels
 *   [n_views + 1] measured lattice pixels that no view sees
 * over the LATTICE of gs_seed: pixels (x, y) with x % stride == stride / 2 and y % stride == stride / 2.
 * One point, in fp32 with one rounding per operation (division and square root correctly rounded; a float32 restatement
 * decides identically; csrc/overlap_point.h is the text, compilable for the host):
 *   the world point is the one gs_seed_apply writes for the pixel:
 *     u = (x + left - padW / 2 + 0.5) / focal_x, v likewise;  z_cam = z / sqrt(u u + v v + 1);
 *     p = rot^T ((u z_cam, v z_cam, z_cam) - tran)
 *   view k:  q = rot_k p + tran_k, each row summed left to right;  cx = padW_k / 2 - left_k, cy likewise (small exact numbers);
 *     seen  <=>  q.z > near  and  fl(fx_k q.x) >= fl((border - cx) q.z)  and  fl(fx_k q.x) < fl((W_k - border - cx) q.z)
 *                and the same two for y
 *   -- the point lies beyond `near` in front of the view and falls on a pixel of its image at least `border` pixels from
 *   every side: the inverse of the renderer's pixel coordinate, cross-multiplied, no division.
 * Two launches on `stream`, no atomics: per-workgroup partial counts go to the workspace as rows of uint32, a second kernel
 * adds them per view in int64.  The result is a pure function of the inputs, whatever the workspace and counts_dev held.
 * Refused before anything is enqueued (GS_E_INVALID, gs_last_error): a null pointer, a frame of non-positive size or focal
 * length, stride < 1, near <= 0 or NaN, border < 0, n_views < 1 or > GS_OVERLAP_MAX_VIEWS, a misaligned or too-small
 * workspace.  The rows of views_dev are in device memory and cannot be validated here without a read: the owner of the table
 * validates each row when it appends it -- gs_view_overlap_check_view (host only, nothing enqueued) refuses a view of
 * non-positive size or focal length and a border with 2 border >= the view's width or height; gs_slam.KeyframeSet calls it. */
#define GS_OVERLAP_MAX_VIEWS 256
typedef struct gs_overlap_opts {
    int32_t stride;   /* >= 1: the lattice of gs_seed (x % stride == stride / 2, y likewise) */
    float   near;     /* > 0: a point counts for a view only with camera z > near         */
    int32_t border;   /* >= 0: pixels taken off each side of a view's image               */
} gs_overlap_opts;
size_t gs_view_overlap_workspace_bytes(int32_t H, int32_t W, int32_t stride, int32_t n_views);
int gs_view_overlap_check_view(const gs_seed_camera *view, int32_t border);
int gs_view_overlap(const float *range, const gs_seed_camera *cam,        /* the incoming frame, by value (host) */
                    const gs_seed_camera *views_dev, int32_t n_views,     /* DEVICE array, 64 bytes per view     */
                    const gs_overlap_opts *opts, int64_t *counts_dev,     /* [n_views + 2]                       */
                    void *workspace, size_t workspace_bytes, gs_stream_t stream);
/* gs_view_overlap with off-centre principal points.  cam: the incoming frame's camera with its offset (its points are those
 * gs_seed_apply_pp writes).  views_dev: the same table of 64-byte rows; view_pp_dev: a DEVICE array of n_views rows of two floats
 * (pp_dx_k, pp_dy_k), 8-byte aligned, or NULL when no view has an offset.  View k's test moves its four bounds by its own
 * offset, in fp32 with one rounding per operation (csrc/overlap_point.h is the text):
 *   fl(fx_k q.x) >= fl(fl((float)(border - cx0_k) - pp_dx_k) q.z)  and  fl(fx_k q.x) < fl(fl((float)(W_k - border - cx0_k) - pp_dx_k) q.z)
 * and the same two for y.  A call in which no camera has an offset -- cam's is (0, 0) and view_pp_dev is NULL -- IS
 * gs_view_overlap: the same kernel on the same rows.  Workspace, counts and refusals as gs_view_overlap; also refused: an
 * offset of `cam` that is not finite, a misaligned view_pp_dev.  (The rows of view_pp_dev are validated by the table's owner.) */
int gs_view_overlap_pp(const float *range, const gs_seed_camera_pp *cam, const gs_seed_camera *views_dev,
                       const float *view_pp_dev, int32_t n_views, const gs_overlap_opts *opts, int64_t *counts_dev,
                       void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- redundancy: of the surface points ONE view measured, how many of the other views see each? ----
 * gs_view_overlap counts per view; this counts per point, which is what culling a keyframe asks ("nearly all it measured is
 * seen by at least m others").  range [H,W] and cam: the SOURCE view's own range map and posed camera (by value, on the
 * host), as gs_view_overlap's frame.  views_dev: the same DEVICE table of 64-byte rows gs_view_overlap reads; self_index: the
 * row to leave out -- the source's own row in that table -- or -1 to leave none out.
 * The points are the measured pixels of the `stride` lattice of range, back-projected as gs_view_overlap does
 * (gs_overlap_point of csrc/overlap_point.h).  For each point, c = the number of rows k != self_index, k < n_views, with
 * gs_overlap_seen(p, views[k], near, border) true -- the decision of gs_view_overlap, bit for bit.  hist_dev
 * [GS_REDUNDANCY_BINS + 1] int64 on the device, 8-byte aligned:
 *   [b], b < 7   measured lattice pixels with c == b
 *   [7]          measured lattice pixels with c >= 7
 *   [8]          measured lattice pixels (the sum of the eight bins)
 * Two launches on `stream`, no atomics and no host synchronisation: a count kernel writes one row of nine uint32 partial
 * counts per workgroup to the workspace, a finalize kernel adds the rows in int64 in a fixed order.  The result is a pure
 * function of the inputs, whatever hist_dev and the workspace held.  n_views == 1 with self_index == 0 is valid: every
 * measured point lands in bin 0.
 * Refused before anything is enqueued (GS_E_INVALID, gs_last_error): everything gs_view_overlap refuses (a null pointer, a
 * source of non-positive size or focal length, stride < 1, near <= 0 or NaN, border < 0, n_views < 1 or >
 * GS_OVERLAP_MAX_VIEWS, a misaligned views_dev, a misaligned or too-small workspace), self_index outside [-1, n_views), a
 * misaligned hist_dev.  The rows of views_dev are validated by the table's owner (gs_view_overlap_check_view).
 * gs_view_redundancy_pp: off-centre principal points, as gs_view_overlap_pp -- cam carries the source's offset, view_pp_dev
 * the views' (two floats a row, 8-byte aligned, or NULL), the *_pp decisions are taken; with no offset anywhere the call IS
 * gs_view_redundancy.  Also refused: an offset of `cam` that is not finite, a misaligned view_pp_dev. */
#define GS_REDUNDANCY_BINS 8
size_t gs_view_redundancy_workspace_bytes(int32_t H, int32_t W, int32_t stride);
int gs_view_redundancy(const float *range, const gs_seed_camera *cam,      /* the SOURCE view: its range map, its camera (host) */
                       const gs_seed_camera *views_dev, int32_t n_views,   /* the same DEVICE table gs_view_overlap reads        */
                       int32_t self_index,                                 /* row to leave out, or -1: none                      */
                       const gs_overlap_opts *opts, int64_t *hist_dev,     /* [GS_REDUNDANCY_BINS + 1]                           */
                       void *workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_view_redundancy_pp(const float *range, const gs_seed_camera_pp *cam, const gs_seed_camera *views_dev,
                          const float *view_pp_dev, int32_t n_views, int32_t self_index, const gs_overlap_opts *opts,
                          int64_t *hist_dev, void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- editing the map: remove rows by one per-row decision, move everything that shares the row index ----
 * Two calls around one host read, because the caller sizes the destination arrays between them (as gs_densify_* and
 * gs_seed_*):
 *   gs_prune_classify: decides every row and writes counts_dev[2] = (kept, removed);
 *   gs_prune_apply   : the kept row with kept-rank r (the number of kept rows before it: the compaction is stable) goes to row
 *                      dst_offset + r of EVERY dst[k]; rows in front of dst_offset and behind dst_offset + kept are not
 *                      touched.  Nothing is written if dst_offset + kept > capacity (counts_dev still holds the need).
 * The decision, in fp32 with one rounding per operation (a float32 restatement decides identically up to expf):
 *   keep  <=>  opa[i] > opa_logit_min  and  norm < scale_max
 *   norm = sqrtf(a a + b b + c c),  (a, b, c) = |scale[i]| per axis (scale_activation 0) or expf(scale[i]) (1)
 * -- the delete rule of gs_densify_classify with both thresholds as arguments (there: logit(0.02) and delete_thresh).  A NaN
 * in opa[i] or scale[i] means not kept.  scale_max = +inf switches the second test off for every finite norm (a norm that
 * overflowed to +inf is still not kept).  opa is the raw logit; a caller that thinks in probabilities converts on the host.
 * arrays: up to GS_PRUNE_MAX_ARRAYS arrays of fp32 rows, N rows in each src, `capacity` rows in each dst, any width >= 1
 * (1, 3, 4, 27 and 48 occur); every array is moved by the same kernel in the same launch: a workgroup writes the destination
 * span of its 256 source rows with consecutive lanes on consecutive floats, whatever the width.  No dst may be a src (the
 * move is not in place) and no dst may overlap any src (not checked beyond equality).  Ranks come from wave ballots,
 * per-workgroup counts and a scan -- no atomics: the result is a pure function of the inputs, whatever the workspace held.
 * The same workspace goes to both calls (8-byte aligned, gs_prune_workspace_bytes(N): one bit and an eighth of a count per
 * row).  Refused before anything is enqueued (GS_E_INVALID, gs_last_error): a null pointer (a src may be null only with
 * N = 0, a dst only with capacity = 0), N < 0 or >= 2^31, n outside 1 .. GS_PRUNE_MAX_ARRAYS, a width < 1, a dst[k] equal to a
 * src[j], a non-finite opa_logit_min, a NaN scale_max, an unknown activation, a misaligned or too-small workspace, a negative
 * dst_offset or capacity.  N = 0 is valid: counts (0, 0), nothing moves.  All launches on `stream`. */
#define GS_PRUNE_MAX_ARRAYS 16
typedef struct gs_prune_opts {
    float opa_logit_min;      /* keep needs opa[i] > this (raw logit; finite)                                   */
    float scale_max;          /* keep needs ||act(scale[i])|| < this; +inf switches the test off                */
    int32_t scale_activation; /* 0 = abs, 1 = exp                                                               */
} gs_prune_opts;
typedef struct gs_prune_arrays {   /* n arrays of fp32 rows that share the row index */
    int32_t n;                     /* 1 .. GS_PRUNE_MAX_ARRAYS */
    int32_t width[GS_PRUNE_MAX_ARRAYS];     /* floats per row, >= 1 */
    const float *src[GS_PRUNE_MAX_ARRAYS];  /* N rows each */
    float *dst[GS_PRUNE_MAX_ARRAYS];        /* `capacity` rows each; must not overlap any src */
} gs_prune_arrays;
size_t gs_prune_workspace_bytes(int64_t N);
int gs_prune_classify(const float *scale, const float *opa, int64_t N, const gs_prune_opts *opts, int64_t *counts_dev,
                      void *workspace, size_t workspace_bytes, gs_stream_t stream);
int gs_prune_apply(const gs_prune_arrays *arrays, int64_t N, int64_t dst_offset, int64_t capacity,
                   const int64_t *counts_dev, const void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- densification, continued: whatever shares the row index follows the edit of gs_densify_apply ----
 * (declared here because it takes gs_prune_arrays as it stands: n arrays of fp32 rows that share the row index.)
 * Takes the workspace and counts_dev that gs_densify_classify wrote for these N rows and follows that call as
 * gs_densify_apply does; neither disturbs the other and the order between the two is free.  With (K, C, S) = counts_dev[0..2]
 * and kept_rank(i) the number of non-deleted rows before row i, for every array k:
 *   row i kept, or kept and cloned (gs_densify_apply leaves the row itself unchanged): dst[k][kept_rank(i)] = src[k][i]
 *   row i split (its kept slot holds a new sample at a new scale)                    : dst[k][kept_rank(i)] = 0
 *   row i deleted                                                                    : nothing
 *   destination rows [K, K + C + S) (the clones, the second split samples)           : 0
 * Every row of [0, K + C + S) of every dst[k] is written exactly once; rows at and beyond K + C + S are not touched; nothing
 * at all is written when the total exceeds `capacity` (gs_densify_apply's rule).  The result is a pure function of the
 * inputs, whatever dst held: one launch for all arrays, no atomics, bitwise repeatable.  A workgroup's 256 source rows own
 * three contiguous destination spans (kept, clone, second sample) and consecutive lanes walk consecutive floats of each,
 * whatever the width (1, 3, 4, 27 and 48 occur) -- gs_prune_apply's way.  Meant for Adam's moment arrays: a zero-moment row
 * takes a first step of a fresh Adam's magnitude.
 * Refused before anything is enqueued (GS_E_INVALID, gs_last_error), as gs_prune_apply: a null pointer (a src may be null only
 * with N = 0, a dst only with capacity = 0), N < 0 or >= 2^31, n outside 1 .. GS_PRUNE_MAX_ARRAYS, a width < 1, a dst[k] equal
 * to a src[j], a missing, misaligned (4 bytes) or too-small workspace (gs_densify_workspace_bytes(N)), a negative capacity.
 * N = 0 is valid and moves nothing. */
int gs_densify_apply_state(const gs_prune_arrays *arrays, int64_t N, int64_t capacity, const int64_t *counts_dev,
                           const void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- per-Gaussian contributions: each Gaussian's share of a rendered frame ----
 * For a TRAINING frame that gs_frame_forward has rendered (any colour model, with or without GS_FRAME_AUX,
 * GS_FRAME_PRINCIPAL_POINT, GS_FRAME_LONG_SORT, GS_FRAME_LONG_LISTS, any listing method), a pixel p of the CROPPED height x width
 * image (pixels of the padded border count for nothing) and a Gaussian g listed in the tile of p:
 *   w_g(p) = alpha_g(p) T_g(p)
 * with exactly the expressions of the compositing kernels: alpha = 2^-(q + nlop), nlop = -log2 sigmoid(opa), and the masked
 * transmittance, which is exactly 0 once the pixel has reached the 1e-4 stop -- what the raster backward recomputes from a
 * bucket's checkpoint.  For a list entry the forward did not process (its key lies behind the tile's stop key), w = 0.
 * One 16-byte row per Gaussian:
 *   weight_sum = sum_p w_g(p),  weight_max = max_p w_g(p),  pixels = #{p : w_g(p) >= w_min},  views = pixels > 0 ? 1 : 0.
 * The row of a culled Gaussian is all zeros; so is every row of a frame that overflowed its pair capacity (it is rendered
 * empty).  N = 0 is valid: nothing is written.  accumulate = 1 combines the row with what `rows` holds: +=, max, +=, += --
 * `views` then counts the frames in which the Gaussian reached w_min somewhere.  Sums run in a fixed order and without
 * atomics (a fixed tree over a tile's pixels, then the Gaussian's tiles in ascending row order): two calls give the same bytes,
 * whatever the workspace held.
 * Must follow a gs_frame_forward with training=1 on the same workspace, in the stream order a gs_frame_backward would: behind
 * that forward, in front of the next forward of the workspace.  It writes nothing a later gs_frame_backward / _part / _adam*
 * of the frame reads, except a bucket work list identical to the one that backward builds: their outputs are the bits they
 * are without this call.
 * workspace: 256-byte aligned, gs_frame_contrib_workspace_bytes(f->max_pairs) (16 bytes per pair; monotone in max_pairs).
 * Refused before anything is enqueued (GS_E_INVALID, gs_last_error): a frame that is not a training frame, rows NULL with
 * N > 0 or not 16-byte aligned, w_min NaN, <= 0 or > 1, accumulate outside {0, 1}, a NULL opts, a misaligned or too-small
 * workspace; and whatever gs_frame_forward refuses of the description. */
typedef struct gs_contrib_row { float weight_sum, weight_max; uint32_t pixels, views; } gs_contrib_row;
typedef struct gs_contrib_opts { float w_min; int32_t accumulate; } gs_contrib_opts;
size_t gs_frame_contrib_workspace_bytes(int64_t max_pairs);
int gs_frame_contrib(const gs_frame *f, const gs_contrib_opts *opts, gs_contrib_row *rows /* [N] device */,
                     void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* gs_prune_classify with the contribution rule joined to it: a row is kept iff gs_prune_classify would keep it AND
 * rows[i].weight_max >= weight_max_min AND rows[i].pixels >= pixels_min AND rows[i].views >= views_min (a NaN weight_max: not
 * kept).  The workspace and counts_dev are written in exactly gs_prune_classify's format: gs_prune_apply follows unchanged,
 * and copts = {0.f, 0, 0} decides what gs_prune_classify decides.  Refusals: gs_prune_classify's, a NULL rows (with N > 0)
 * or copts, a NaN or negative weight_max_min. */
typedef struct gs_prune_contrib_opts { float weight_max_min; uint32_t pixels_min, views_min; } gs_prune_contrib_opts;
int gs_prune_classify_contrib(const float *scale, const float *opa, const gs_contrib_row *rows, int64_t N,
                              const gs_prune_opts *opts, const gs_prune_contrib_opts *copts, int64_t *counts_dev,
                              void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- point-to-plane ICP: align an incoming range map to the map's depth, solved on the device ----
 * The map is rendered ONCE, at the predicted pose (GS_FRAME_AUX: depth D and alpha A); gs_icp_model_maps turns those maps into
 * a vertex map and a normal map in that camera's frame.  After that an iteration (gs_icp_step) is one pass over the incoming
 * frame's range map and a 6 x 6 solve: no rendering, no backward, no host read.  The unknown is the rigid motion
 * p_model = R p_frame + t between the two camera frames, kept in double in a small device state.
 * Cameras are gs_seed_camera_pp; only the sizes, focal lengths and offsets are read (the maps live in their camera's own frame).
 * "No measurement" is the rule of gs_view_overlap: a range counts where it is > 0 and finite.
 * The per-pixel rule, in fp32 with one rounding per operation (division and square root correctly rounded; a float32
 * restatement computes every vertex, normal and keep / drop decision alike; csrc/icp_point.h is the text, compilable for the
 * host):
 *   ray of pixel (x, y):  u = fl(fl(fl((float)(x + left - padW / 2) + 0.5f) - pp_dx) / focal_x),  v likewise  (the ray of
 *                         gs_seed_apply_pp and gs_view_overlap_pp; offsets (0, 0) give the bits of the centred ray)
 *   point at range z:     zc = z / sqrt(u u + v v + 1);  p = (u zc, v zc, zc)
 *   model maps:           rho = D / A where A >= alpha_min, else no measurement (alpha == NULL: rho = D, a plain range map);
 *                         vertex = point(rho) with w = 1 where rho is measured, else (0, 0, 0, 0);
 *                         normal = normalize((v[x+s] - v[x-s]) x (v[y+s] - v[y-s])), s = normal_step, negated where n.v > 0,
 *                         with w = 1 only where the pixel and its four neighbours are inside the image and measured, their
 *                         largest range hi <= fl(fl(1 + edge_rel) lo) of their smallest (edge_rel < 0: no edge test; the edge
 *                         rule of gs_pyramid_down: a stencil across a depth edge has no normal) and the cross product's length
 *                         is > 0 and finite; else (0, 0, 0, 0)
 *   step, per measured LATTICE pixel (x % stride == stride / 2, y likewise: the lattice of gs_seed):
 *                         q = R p + t, each row summed left to right, the state rounded to fp32 once;
 *                         model pixel: f = fl(fl(fl(fx_m fl(q.x / q.z)) + pp_dx_m) - (float)(left_m - padW_m / 2)), i = floor(f)
 *                         (pixel i covers [i, i + 1): the inverse of the renderer's pixel coordinate), j likewise;
 *                         kept  <=>  q.z > 0  and  0 <= f < W_m (and y)  and  the normal at (i, j) has w = 1
 *                                    and  |q - v|^2 <= fl(dist_max dist_max)  and  -(n.v) >= fl(cos_min |v|)
 *                         e = n.(q - v),  J = (q x n, n)
 * gs_icp_step, two launches: the first accumulates, over the kept pixels, the 21 upper entries of J J^T (row-major), the 6 of
 * J e and e e, and counts the kept and the measured lattice pixels -- per thread (one term per chunk of its workgroup's run),
 * a butterfly per wave, the waves in index order, one 32-float row per workgroup in the workspace; no atomics.  The grid is
 * capped at 1,024 workgroups of 256: a frame with more than 262,144 lattice pixels gives each workgroup a run of several
 * chunks.  The second launch is one workgroup: it adds the rows in double in a fixed order, solves
 *   (A + damping tr(A) / 6 I) x = -b,  A = sum J J^T,  b = sum J e,  x = (x_w, x_t)
 * by Cholesky in double, applies R <- exp([x_w]x) R, t <- exp([x_w]x) t + x_t, adds one to state.iteration and writes row
 * `log_row` of the log, GS_ICP_LOG_DOUBLES doubles:
 *   [0] kept  [1] measured lattice pixels  [2] sum e e  [3..23] A (21 upper entries)  [24..29] b  [30..35] x  [36] status
 *   [37] damping tr(A) / 6  [38] stride  [39] 0
 * status GS_ICP_TOO_FEW (kept < min_count) or GS_ICP_NOT_POSITIVE (a pivot that is not positive and finite, or a solution
 * that is not finite): R and t stay bit for bit, x is written as zeros.  The result is a pure function of the inputs,
 * whatever the workspace held.  gs_icp_reset writes a state (iteration 0) and zeroes a log of `log_rows` rows, on the stream.
 * vertex / normal: [H, W] float4 each, gs_icp_model_bytes(H, W) bytes each, 16-byte aligned.  workspace: 16-byte aligned,
 * gs_icp_workspace_bytes(H, W, stride) of the FRAME's size (monotone in the image, falling with the stride).  log:
 * gs_icp_log_bytes(rows).  The size queries return 0 for arguments the calls refuse.
 * Refused before anything is enqueued (GS_E_INVALID, gs_last_error): a null pointer (alpha may be NULL), a non-positive size or
 * focal length, an offset that is not finite, stride < 1, normal_step < 1, dist_max <= 0 or NaN, a NaN cos_min, alpha_min or
 * edge_rel, a negative or non-finite damping, a negative min_count, misaligned maps, state or log, a misaligned or too-small
 * workspace, log_row outside [0, log_rows) -- a full log --, a rot or tran of gs_icp_reset that is not finite. */
#define GS_ICP_LOG_DOUBLES 40
#define GS_ICP_OK 0
#define GS_ICP_TOO_FEW 1
#define GS_ICP_NOT_POSITIVE 2
typedef struct gs_icp_model_opts {
    float alpha_min;     /* the model has a surface where its alpha reaches this                        */
    float edge_rel;      /* < 0: off; else a normal's stencil counts only where hi <= (1 + edge_rel) lo */
    int32_t normal_step; /* >= 1: the central difference reaches this many pixels to each side          */
} gs_icp_model_opts;
typedef struct gs_icp_opts {
    int32_t stride;      /* >= 1: the lattice of gs_seed over the incoming frame                        */
    float dist_max;      /* > 0: a pair counts only within this distance                                */
    float cos_min;       /* ... and where the model surface faces its own ray at least this much        */
    int32_t min_count;   /* fewer kept pixels: no step, status GS_ICP_TOO_FEW                           */
    double damping;      /* >= 0: x the mean diagonal of A, added to the diagonal                       */
} gs_icp_opts;
typedef struct gs_icp_state { /* on the DEVICE */
    double R[9], t[3];   /* p_model = R p_frame + t (row-major)                                         */
    int32_t iteration;   /* steps taken since gs_icp_reset                                              */
    int32_t reserved;
} gs_icp_state;
size_t gs_icp_model_bytes(int32_t H, int32_t W);
size_t gs_icp_workspace_bytes(int32_t H, int32_t W, int32_t stride);
size_t gs_icp_log_bytes(int32_t rows);
int gs_icp_model_maps(const float *depth, const float *alpha, const gs_seed_camera_pp *cam, const gs_icp_model_opts *opts,
                      float *vertex, float *normal, gs_stream_t stream);
int gs_icp_reset(gs_icp_state *state_dev, double *log_dev, int32_t log_rows, const double *rot /* [9] host */,
                 const double *tran /* [3] host */, gs_stream_t stream);
int gs_icp_step(const float *range, const gs_seed_camera_pp *cam,           /* the incoming frame            */
                const float *vertex, const float *normal, const gs_seed_camera_pp *model_cam, /* gs_icp_model_maps' */
                const gs_icp_opts *opts, gs_icp_state *state_dev, double *log_dev, int32_t log_rows, int32_t log_row,
                void *workspace, size_t workspace_bytes, gs_stream_t stream);

/* ---- the pose of a tracked frame, stepped on the device (pose_step.hip): what gs_frame_forward / gs_frame_backward_pose of a
 * GS_FRAME_DEVICE_POSE frame read and write between them, so that a whole tracking call is enqueued without a host wait.
 * gs_pose_step is gs_track.PoseAdam.step, so3_exp, rot_tangent_grad and the best-pose bookkeeping of Tracker.track in double:
 * ONE launch of one wave, no atomics, every store a plain store from a vector lane, a pure function of its inputs.
 * One step, in this order:
 *   the log row `log_row` = (the 12 floats of pose_dev as the frame just rendered them, grad_rot[9], grad_tran[3], the
 *     n_values floats of values_dev): GS_POSE_LOG_HEAD + n_values floats;
 *   *skip_if_nonzero != 0 (8 bytes: gs_frame_overflow_flag's counter; NULL: never) -> skipped += 1, the row's loss
 *     (value 0) is NaN and nothing else changes;
 *   else any of the 12 gradients or values[0] not finite -> bad += 1 and nothing else changes;
 *   else: track_best and values[0] < best_loss -> best_R / best_t = R / t (the pose BEFORE the step), best_loss = values[0],
 *     best_row = log_row; then g = (dL/dw at w = 0 of exp([w]x) R from G = grad_rot: with M = G R^T, (M21 - M12, M02 - M20,
 *     M10 - M01), grad_tran); steps += 1; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; d = lr lr_scale (m / (1 - b1^steps))
 *     / (sqrt(v / (1 - b2^steps)) + eps); R <- exp([-d_w]x) R (Rodrigues; the series I + K + K K / 2 below 1e-8 rad),
 *     t <- t - d_t; pose_dev <- (float)(R, t), each entry rounded to fp32 once.
 * gs_pose_reset writes the state (the pose, zero moments and counters, best = the pose with best_loss = +inf and best_row
 * -1), pose_dev = (float)(rot, tran) and zeroes the log, all on the stream.
 * GS_E_INVALID, before anything is enqueued: a null pointer (skip_if_nonzero alone may be NULL); a rot / tran of gs_pose_reset
 * that is not finite; lr_rot, lr_tran, lr_scale or eps not positive and finite; a beta outside [0, 1); n_values other than 4
 * or 8; log_rows < 1; log_row outside [0, log_rows); state_dev or skip_if_nonzero not 8-byte, pose_dev or log_dev not 16-byte,
 * a gradient or values_dev not 4-byte aligned. */
#define GS_POSE_LOG_HEAD 24
typedef struct gs_pose_state { /* on the DEVICE */
    double R[9], t[3];        /* the current pose, world -> camera; R on SO(3) by construction                */
    double m[6], v[6];        /* Adam's moments on (w, tran)                                                  */
    double best_R[9], best_t[3], best_loss; /* the lowest-loss pose among the rows with track_best set        */
    int32_t steps;            /* steps taken since gs_pose_reset                                              */
    int32_t best_row;         /* the log row of `best`; -1: none yet                                          */
    int32_t skipped;          /* calls that found *skip_if_nonzero set (the frame overflowed its workspace)   */
    int32_t bad;              /* calls that found a gradient or the loss not finite                           */
} gs_pose_state;
typedef struct gs_pose_step_opts {
    double lr_rot, lr_tran, lr_scale, beta1, beta2, eps;
    int32_t track_best;       /* does this call's loss compete for `best`? (the last stage of a schedule)     */
    int32_t n_values;         /* floats of values_dev: 4 (gs_loss_track) or 8 (gs_loss_track_gated)           */
} gs_pose_step_opts;
size_t gs_pose_log_bytes(int32_t rows, int32_t n_values); /* 0 on bad arguments */
int gs_pose_reset(gs_pose_state *state_dev, float *pose_dev, float *log_dev, int32_t log_rows, int32_t n_values,
                  const double *rot /* [9] host */, const double *tran /* [3] host */, gs_stream_t stream);
int gs_pose_step(const float *grad_rot_dev, const float *grad_tran_dev, const float *values_dev,
                 const void *skip_if_nonzero, const gs_pose_step_opts *opts, gs_pose_state *state_dev, float *pose_dev,
                 float *log_dev, int32_t log_rows, int32_t log_row, gs_stream_t stream);

/* ---- a view's affine exposure (exposure.hip): six numbers per view in device memory, exposure_dev = gain[3] then bias[3],
 * contiguous fp32, read by the kernels as they stand when the kernels run (as a GS_FRAME_DEVICE_POSE frame reads its pose).
 * Every colour loss of this section is taken on the compensated image I' in place of the rendered I; depth and alpha terms
 * are untouched.  All arithmetic on the maps is fp32 with one rounding per operation, no contraction:
 *   gs_exposure_apply   : out_pc = fl(fl(gain_c image_pc) + bias_c); image, out [H,W,3].  One streaming pass, one launch.  The
 *     identity (1,1,1,0,0,0) gives out = image bit for bit (a -0 element alone becomes +0).  out may not overlap image: the
 *     backward needs I.
 *   gs_exposure_backward: on entry grad [H,W,3] holds g' = dL/dI' (what a loss kernel wrote), on exit g_pc = fl(gain_c g'_pc)
 *     (what the frame backward takes; the identity leaves it bit for bit).  grad_exposure_out (6 floats on the device; may be
 *     NULL) = (dL/dgain_c = sum_p g'_pc image_pc, dL/dbias_c = sum_p g'_pc): each product in double from its two fp32 operands,
 *     summed in double per thread in pixel order, per wave, per workgroup and by one last workgroup over the workgroups' rows
 *     in a fixed order, each total rounded to fp32 once.  No atomics: bitwise repeatable.
 *     adam (may be NULL): the same last workgroup then takes ONE Adam step on the six numbers in double, on the six fp32
 *     gradients just formed g: steps += 1; m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g; d = (lr lr_scale (m / (1 -
 *     b1^steps))) / (sqrt(v / (1 - b2^steps)) + eps), lr = lr_gain for the gains and lr_bias for the biases; exposure_dev[k] =
 *     (float)((double)exposure_dev[k] - d).  It is a second launch: every read of the gain precedes the write.  No step --
 *     state and numbers untouched bit for bit -- where *skip_if_nonzero != 0 (8 bytes on the device, the meaning of
 *     gs_adam_fused.skip_if_nonzero; NULL: never) or one of the six gradients is not finite.  With adam NULL exposure_dev is
 *     not written.  With grad_exposure_out and adam both NULL no sum is formed: one launch.
 * GS_E_INVALID, before anything is enqueued: a null image, grad, out or exposure_dev; a map not 16-byte, exposure_dev or
 * grad_exposure_out not 4-byte, state or skip_if_nonzero not 8-byte aligned; H or W <= 0; out or grad overlapping image; a
 * null state; lr_gain, lr_bias, lr_scale or eps negative, NaN or infinite; a beta outside [0, 1); a workspace that is null,
 * not 8-byte aligned or smaller than gs_exposure_workspace_bytes(H, W) (48 bytes per 1,024 pixels). */
typedef struct gs_exposure_state { /* on the DEVICE, 104 bytes; all zero = a fresh optimizer */
    double m[6], v[6];        /* Adam's moments on (gain[3], bias[3])                                         */
    double steps;             /* steps taken                                                                  */
} gs_exposure_state;
typedef struct gs_exposure_adam {
    gs_exposure_state *state; /* device                                                                       */
    double lr_gain, lr_bias, beta1, beta2, eps, lr_scale;
    const void *skip_if_nonzero; /* device, 8 bytes; may be NULL                                              */
} gs_exposure_adam;
size_t gs_exposure_workspace_bytes(int32_t H, int32_t W); /* 0 on bad arguments */
int gs_exposure_apply(const float *image, const float *exposure_dev, int32_t H, int32_t W, float *out, gs_stream_t stream);
int gs_exposure_backward(const float *image, float *grad, float *exposure_dev, int32_t H, int32_t W, float *grad_exposure_out,
                         const gs_exposure_adam *adam, void *workspace, size_t workspace_bytes, gs_stream_t stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GS_ABI_H */
