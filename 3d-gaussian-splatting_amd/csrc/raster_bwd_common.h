// raster_bwd_common.h -- what the files of the tile rasterizer backward share: the kernels' argument structs, the pixel
// inputs, the grid of the one-wave-per-bucket kernels and the host functions the files call across their boundaries.
// The overview of the kernels and the gradient identities: raster_bwd.hip.
#pragma once
#include "raster_common.h"

// (at namespace scope, like RasterSrc / RasterGeom: the launch functions below take them across files)
struct BwdOut {
    // FRAME: one row per pair, addressed in EMISSION order (pair_offsets[g] + index of the tile
    // inside g's rectangle), so the per-Gaussian sum is a contiguous, deterministic reduction
    float *rows;                   // [max_pairs][16 | 48 | 64]: gs_frame_layout.h (gs_row_floats, gs_row_geo, gs_row_col)
    uint32_t *exec_rows;           // SH backward on the matrix pipe: pixel-row steps executed per (workgroup, wave)
    const uint32_t *pair_offsets;  // [N]
    const uint4 *rects;            // [N]
    uint64_t max_pairs;
    // REF: one row per pair
    float *grad_pos, *grad_rgb, *grad_opa, *grad_cov;
};

struct BwdIn {
    const float *c_final;     // padded image [padH,padW,3]
    const float *grad;        // FRAME: dL/d(cropped, clamped image) [H,W,3]; REF: [padH,padW,3]
    const float4 *ckpt;
    const uint32_t *tile_nproc;
    const uint32_t *bucket_offsets;  // [T+1]
    const uint4 *bucket_info;        // [n_buckets] (tile, first Gaussian, count, start of the tile's list)
    const int32_t *ranges;           // FRAME: [T][2]; REF: accum [T+1]
    const uint32_t *tile_order;      // FRAME, optional: the tiles in descending order of their cost (one workgroup per tile)
    // Always 0.  What is left of the long-list hand-over that work items replaced (round 5): the one-wave-per-bucket kernels
    // skip a tile's buckets below this index.  Kept for the register allocation alone: without this uniform test in
    // raster_backward_pixel_sh_body five of the ten kernels built from it get more spills (the rgb training kernel its first
    // two spilled VGPRs; HISTORY.md, the listing at the end of profiles/dead_paths_isa_diff.txt).  To go with the next retuning of that kernel.
    uint32_t skip_buckets;
    uint32_t use_rows;  // rgb frames: GS_FRAME_BWD_ROWS -- the row-layout kernel instead of the pixel-parallel one (gs_stage_raster_backward)
    // SH frames on the matrix pipe: the work items (tile, first bucket, buckets) of mfma_items_kernel and their count
    const uint4 *mfma_items;
    const uint32_t *mfma_n_items;
};

// Inputs of one pixel for the backward kernels: final colour, and dL/dC -- for the frame path the gradient of
// the clamped + cropped output (splatter.py:652-653: zero outside the crop and where the colour was clamped).
// The gradient is loaded unconditionally and masked afterwards: a load that depends on c_final's value would
// serialise two memory round trips.
template <bool FRAME>
__device__ __forceinline__ void load_pixel_inputs(const BwdIn &I, const RasterGeom &G, uint32_t id_x, uint32_t id_y,
                                                  float f[3], float g[3]) {
    const float *cf = I.c_final + ((size_t)id_y * G.padW + id_x) * 3;
    f[0] = cf[0];
    f[1] = cf[1];
    f[2] = cf[2];
    if (FRAME) {
        const int ox = (int)id_x - G.crop_left, oy = (int)id_y - G.crop_top;
        const bool in = ox >= 0 && ox < G.width && oy >= 0 && oy < G.height;
        const float *gp = I.grad + ((size_t)(in ? oy : 0) * G.width + (in ? ox : 0)) * 3;
        const float u0 = gp[0], u1 = gp[1], u2 = gp[2];
        g[0] = (in && f[0] >= 0.f && f[0] <= 1.f) ? u0 : 0.f;
        g[1] = (in && f[1] >= 0.f && f[1] <= 1.f) ? u1 : 0.f;
        g[2] = (in && f[2] >= 0.f && f[2] <= 1.f) ? u2 : 0.f;
    } else {
        const float *gp = I.grad + ((size_t)id_y * G.padW + id_x) * 3;
        g[0] = gp[0];
        g[1] = gp[1];
        g[2] = gp[2];
    }
}

// Inputs of the depth / alpha terms (GS_FRAME_AUX training frames; raster_aux_backward_kernel): the forward's final (D, A)
// sums and its per-bucket (D, A) checkpoints, dL/d(depth) and dL/d(alpha) of the cropped maps (NULL = zero).
struct AuxBwdIn {
    const float2 *padded;
    const float2 *ckpt;
    const float *grad_depth, *grad_alpha;
};

// Grid of the one-wave-per-bucket kernels of the frame path (the pixel-parallel and row-layout backward kernels, and
// contrib.hip's pair kernel): the work list's capacity, but at most GS_BWD_GRID_CAP waves.
// The kernels walk the list with the grid as the stride, so the cap only decides how many waves come up empty (a frame
// whose tiles saturate early fills a third of the capacity) or take a second bucket (a frame beyond the cap: the waves
// are still 8 x the device's resident slots, i.e. fresh waves keep arriving while others are in their load phase -- what
// the measured-and-dropped persistent grids of round 2 lacked).
#ifndef GS_BWD_GRID_CAP
#define GS_BWD_GRID_CAP 40960
#endif
static inline unsigned bwd_frame_grid(int64_t max_buckets) {
    return (unsigned)(max_buckets > 0 ? (max_buckets < GS_BWD_GRID_CAP ? max_buckets : GS_BWD_GRID_CAP) : 1);
}

// ---- what the files hand each other (host) ----
// One launch function per kernel family, defined beside the kernels: it owns the family's grid and block geometry and picks
// the instantiation.  Which family a frame or a reference call gets is decided in raster_bwd.hip alone.  `color_dim` is one
// the caller has validated for the family; `max_buckets` is the capacity of the bucket work list.
// raster_bwd_systolic.hip: `sigmoid = True` of the reference API, rgb or degree-2 SH colours (3 | 27)
void gs_launch_bwd_systolic(int color_dim, int exact, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                            int64_t max_buckets, hipStream_t stream);
// raster_bwd_pixel.hip: the pixel-parallel kernel.  frame: 3 | 27 | 48 on the capped grid; reference API: 3 | 27, a wave per
// bucket of the capacity, `exact` = its `fast = 0` flavour (reference API only)
void gs_launch_bwd_pixel(int color_dim, bool frame, int exact, const RasterSrc &S, const RasterGeom &G, const BwdIn &I,
                         const BwdOut &O, int64_t max_buckets, hipStream_t stream);
// ... and with the depth / alpha terms: GS_FRAME_AUX frames, 3 | 27 | 48
void gs_launch_bwd_aux(int color_dim, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                       const AuxBwdIn &X, int64_t max_buckets, hipStream_t stream);
// raster_bwd_mfma.hip: SH frames (27 | 48) on the matrix pipe, the work items the kernel walks (`order`: the tiles, heavy
// first; NULL: raster order), and the (workgroup, wave) slots its executed-row counters take (0: another colour model)
void gs_launch_bwd_mfma(int color_dim, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                        int64_t max_buckets, hipStream_t stream);
void gs_launch_mfma_items(const uint32_t *tile_nproc, int n_tiles, const uint32_t *order, uint4 *items, uint32_t *n_items,
                          hipStream_t stream);
int gs_bwd_mfma_slots(int color_dim, int n_tiles, int64_t max_buckets);
// raster_bwd_rows.hip: rgb frames flagged GS_FRAME_BWD_ROWS
void gs_launch_bwd_rows(const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O, int64_t max_buckets,
                        hipStream_t stream);
// (gs_raster_forward_ref, the forward that gs_draw_backward replays for the checkpoints: raster_common.h)
