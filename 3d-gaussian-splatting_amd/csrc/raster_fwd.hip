// raster_fwd.hip -- forward compositing of the frame path: gs_stage_raster_forward.
//
// The kernel is raster_fwd_body.h's with FRAME = true: rgb, degree-2 or degree-3 SH colours, training (checkpoints) or
// inference, with (raster_aux_forward_kernel) or without the depth / alpha maps.  A dense frame's long lists go on to
// raster_fwd_segment.hip; the reference API (gs_draw) is raster_fwd_ref.hip.
#include "raster_fwd_body.h"

int gs_stage_raster_forward(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids,
                            hipStream_t stream, bool second_pass) {
    gs_frame_geom FG = gs_frame_geometry(f);
    RasterSrc S;
    RasterGeom G;
    gs_frame_raster_args(f, ws, sorted_ids, S, G);
    // dense frames: tiles still alive after GS_LONG_MIN Gaussians hand the rest of their list to the segment kernels
    // (GS_FRAME_AUX frames walk every list with one wave: the segment kernels carry no depth / alpha)
    const bool aux = (f->flags & GS_FRAME_AUX) != 0;
    const bool dense = gs_frame_long_lists(f, FG.n_tiles) && ws.cont_state != nullptr &&
                       !(f->flags & GS_FRAME_SERIAL_LONG_LISTS) && !aux;
    float4 *cs = dense ? ws.cont_state : nullptr;
    uint32_t *cf = dense ? ws.cont_flag : nullptr;
    // longest-first dispatch: the order is written by the strip variant's project + count launch and the cost is recorded
    // by strip-variant frames only (frames of the other variants neither read the order nor record a cost)
    const bool ordered = gs_frame_uses_strips(f) && f->N > 0 && ws.tile_order != nullptr;
    const uint32_t *order = ordered ? ws.tile_order : nullptr;
    uint32_t *cost = ordered ? ws.tile_cost : nullptr;
    // occlusion cut (gs_frame_layout.h): every INFERENCE frame-path launch leaves the table behind for the next frame of this
    // workspace (a training forward leaves it untouched: the caller must not allow the cull right behind one); a frame
    // whose lists were trimmed by it checks them, and its gated second pass composites the full lists
    const bool culled = gs_frame_occlusion_cull(f);
    const uint32_t *cut_in = culled && !second_pass ? gs_frame_cut_table(f, ws) : nullptr;
    unsigned long long *ranpast = ws.counters + GS_CNT_RANPAST;
    const unsigned long long *gate = second_pass ? ranpast : nullptr;
    // GS_FWD_COMPACT, read per frame: 0 keeps every tile in the full layout to its end (the compact phase of the rgb
    // inference kernel switched off); both settings render the same bits
    uint32_t compact_min = GS_FWD_COMPACT_MIN;
    if (const char *e = getenv("GS_FWD_COMPACT")) {
        if (e[0] == '0' && e[1] == 0) compact_min = 0;
    }
    if (aux) {
        order = fwd_tile_order(order);
        const uint32_t T = (uint32_t)FG.n_tiles;
        const uint32_t grid = fwd_launch_grid(T, gate);
        const gs_frame_aux_ws aw = gs_frame_aux(f);
        AuxFwdOut X = {(float2 *)f->aux_padded, f->depth, f->alpha, aw.ckpt};
        gs_for_color_dim(f->color_dim, [&](auto cd) {
            constexpr int CD = decltype(cd)::value;
            if (f->training)
                hipLaunchKernelGGL((raster_aux_forward_kernel<CD, true>), dim3(grid), dim3(FWD_THREADS), 0, stream, S, G,
                                   ws.tile_ranges, f->image_padded, f->image, ws.ckpt, ws.tile_nproc, T, order, cost, nullptr,
                                   nullptr, ranpast, nullptr, X);
            else
                hipLaunchKernelGGL((raster_aux_forward_kernel<CD, false>), dim3(grid), dim3(FWD_THREADS), 0, stream, S, G,
                                   ws.tile_ranges, f->image_padded, f->image, nullptr, nullptr, T, order, cost, cut_in, ws.cut,
                                   ranpast, gate, X);
        });
    } else {
        gs_for_color_dim(f->color_dim, [&](auto cd) {
            constexpr int CD = decltype(cd)::value;
            if (f->training)
                launch_fwd<CD, true, true, false>(S, G, ws.tile_ranges, f->image_padded, f->image, ws.ckpt, ws.tile_nproc, 0,
                                                  stream, cs, cf, order, cost, nullptr, nullptr, ranpast, nullptr);
            else
                launch_fwd<CD, true, false, false>(S, G, ws.tile_ranges, f->image_padded, f->image, nullptr, nullptr, 0, stream,
                                                   cs, cf, order, cost, cut_in, ws.cut, ranpast, gate, dense ? 0u : compact_min,
                                                   ws.tile_compact);
        });
    }
    GS_CHECK_LAUNCH();
    return dense ? gs_stage_raster_segments(f, ws, S, G, stream) : 0;
}
