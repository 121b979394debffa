// raster_bwd.hip -- tile rasterizer backward: the tiles' lists in buckets of 64 Gaussians.
//
// Replaces draw_backward_kernel (gaussian.cu:440-803).  The reference keeps one pixel per
// thread and, for EVERY Gaussian, reduces 10 (no SH) or 34 (SH) gradient terms across the
// warp with 5-step shuffle trees plus shared-memory atomics -- the reduction is most of its
// runtime -- and walks a tile's whole list in one workgroup.
//
// Here a tile's sorted list is cut into BUCKETS of 64 consecutive Gaussians.  Buckets are independent because
// the forward pass (or its replay for the reference-API entry point) checkpointed every pixel's (T, C_run) at
// each bucket boundary, so long tiles are spread over many CUs instead of serialising one workgroup.  This file
// holds the work lists (bucket list, stop keys), the entry points and the choice of the kernel that works on a
// bucket; each kernel has a file of its own, with its header and its launch function (raster_bwd_common.h):
//
//   * raster_backward_pixel_sh_kernel (raster_bwd_pixel.hip), one wave per bucket: lanes own PIXELS (four each), the
//     bucket's Gaussians are applied front to back, the per-Gaussian sums are reduced over the wave through LDS.  Every
//     colour model of the reference API, rgb frames, and -- as raster_aux_backward_kernel -- every GS_FRAME_AUX frame;
//   * raster_backward_rows_kernel (raster_bwd_rows.hip), one wave per bucket: lanes own GAUSSIANS, a step is one pixel
//     row of the tile.  rgb frames flagged GS_FRAME_BWD_ROWS;
//   * raster_backward_mfma_sh_kernel (raster_bwd_mfma.hip), a workgroup per work item of up to eight buckets of a tile:
//     the row layout with the two SH contractions on the matrix pipe.  SH frames;
//   * raster_backward_kernel (raster_bwd_systolic.hip), `sigmoid = True` of the reference API only (a rarely used
//     flag), a 64-lane SYSTOLIC pipeline: lane l keeps Gaussian l's parameters AND its gradient accumulators (10 + 27 SH sums) in registers,
//     the tile's 256 pixels stream through the lanes: at step t lane l handles pixel t - l.  A pixel's
//     running state (transmittance T, rho = dL/dC . (C_final - C_run), dL/dC, pixel centre: 7 registers) moves
//     from lane l to lane l+1 with one DPP `wave_shr:1` per register; lane 0 is fed from LDS.  No cross-lane
//     reduction and no atomics inside the loop: after 256+63 steps every lane holds the complete sums over
//     the tile's pixels for its Gaussian.
//
// Gradient identities used by all of them (A.8 of SURVEY.md):
//   s = dL/dalpha * alpha,  u = -ln G
//   dL/dx = ln2 (2A' Sx - B' Sy),            Sx = sum s dx, Sy = sum s dy
//   dL/da = (-Syy + 2 d Su)/Pn, dL/db = (Sxy - 2 c Su)/Pn, dL/dc = (Sxy - 2 b Su)/Pn,
//   dL/dd = (-Sxx + 2 a Su)/Pn,              Sxx = sum s dx^2, ..., Su = sum s u
// which is the reference's dP1_d{a,b,c,d} (gaussian.cu:610-621) with the per-Gaussian
// constants factored out of the pixel loop.
#include <stdlib.h>

#include "raster_bwd_common.h"

namespace {

// exclusive scan of ceil(nproc/64) over tiles -> bucket_offsets[T+1], total -> *n_buckets (bucket_scan_kernel, one workgroup),
// then one record per bucket (bucket_fill_kernel, a wave per tile): (tile, first Gaussian of the bucket inside the tile's
// list, Gaussians in the bucket, start of the tile's list) -- a bucket kernel's wave learns everything about its work item
// from ONE load instead of a binary search over the offsets followed by three dependent loads.
// Round 5: with frame ranges the scan also counts the buckets of SATURATED tiles -- tiles whose compositing stopped before the
// end of their list because every pixel had saturated -- and returns the count in the upper half of *n_buckets: the share of
// such buckets is what decides between the two rgb backward kernels (GS_FRAME_BWD_ROWS, include/gs_abi.h), and the caller
// reads the counter back with the frame's other counters anyway.
// Two kernels since the end of round 5: until then the scan's ONE workgroup also stored the records -- 31 k x 16 bytes from one
// CU at 2.4 M Gaussians: 28 us alone, and 91 us where it actually runs, on the side stream underneath the caller's loss kernel
// (kernel trace of whole training steps, profiles/r05_z_*): longer than the loss it was meant to hide under; 62 k and more
// records in a densified scene.
__global__ void __launch_bounds__(1024) bucket_scan_kernel(const uint32_t *__restrict__ tile_nproc, int n_tiles,
                                                          uint32_t *__restrict__ bucket_offsets,
                                                          unsigned long long *__restrict__ n_buckets,
                                                          const int32_t *__restrict__ ranges, int frame_ranges) {
    __shared__ uint32_t s_wave[2][16];
    __shared__ uint32_t s_carry[2];
    if (threadIdx.x < 2) s_carry[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < n_tiles; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t np = i < n_tiles ? tile_nproc[i] : 0;
        const uint32_t v = (np + GS_BUCKET - 1) / GS_BUCKET;
        const bool sat = frame_ranges && i < n_tiles && np < (uint32_t)(ranges[2 * i + 1] - ranges[2 * i]);
        const uint32_t incl = gs_wave_incl_scan_u32(v), sat_sum = gs_wave_sum_u32(sat ? v : 0u);
        if (lane == 63) {
            s_wave[0][wave] = incl;
            s_wave[1][wave] = sat_sum;
        }
        __syncthreads();
        uint32_t woff = 0, sat_all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            woff += w < wave ? s_wave[0][w] : 0;
            sat_all += s_wave[1][w];
        }
        const uint32_t carry = s_carry[0];
        if (i < n_tiles) bucket_offsets[i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) {
            s_carry[0] = carry + woff + incl;
            s_carry[1] += sat_all;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bucket_offsets[n_tiles] = s_carry[0];
        *n_buckets = (unsigned long long)s_carry[0] | ((unsigned long long)s_carry[1] << 32);
    }
}
// the records: a wave per tile, lane b takes the tile's buckets b, b + 64, ... (a pile of a densifying run has hundreds)
__global__ void __launch_bounds__(256) bucket_fill_kernel(const uint32_t *__restrict__ tile_nproc, int n_tiles,
                                                         const uint32_t *__restrict__ bucket_offsets,
                                                         uint4 *__restrict__ bucket_info,
                                                         const int32_t *__restrict__ ranges, int frame_ranges) {
    const int tile = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (tile >= n_tiles) return;
    const uint32_t np = tile_nproc[tile], v = (np + GS_BUCKET - 1) / GS_BUCKET;
    if (v == 0) return;
    const uint32_t first = bucket_offsets[tile], st = (uint32_t)(frame_ranges ? ranges[2 * tile] : ranges[tile]);
    for (uint32_t b = (uint32_t)lane; b < v; b += 64) {
        const uint32_t rem = np - b * GS_BUCKET;
        bucket_info[first + b] = make_uint4((uint32_t)tile, b * GS_BUCKET, rem < GS_BUCKET ? rem : GS_BUCKET, st);
    }
}
static inline void gs_launch_bucket_list(const uint32_t *tile_nproc, int n_tiles, uint32_t *bucket_offsets,
                                         unsigned long long *n_buckets, uint4 *bucket_info, const int32_t *ranges,
                                         int frame_ranges, hipStream_t stream) {
    hipLaunchKernelGGL(bucket_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_nproc, n_tiles, bucket_offsets, n_buckets,
                       ranges, frame_ranges);
    hipLaunchKernelGGL(bucket_fill_kernel, dim3((unsigned)gs_div_up(n_tiles, 4)), dim3(256), 0, stream, tile_nproc, n_tiles,
                       bucket_offsets, bucket_info, ranges, frame_ranges);
}

// Frame path, rgb rows: the key (depth bits, Gaussian) of the last list entry the forward processed in every tile
// (depth 0: none), as two arrays of T 32-bit words.  A tile's list ascends in exactly this key and the key is unique, so "pair (tile, g) was processed --
// its gradient row written" <=> key(g) <= stop_keys[tile]: what the projection backward needs to know about a row
// without a flag per row (no scattered flag stores, no flag memset; gs_frame_layout.h).  One thread per tile, three
// dependent loads; runs with the bucket scan underneath the caller's loss.
__global__ void __launch_bounds__(256) stop_key_kernel(const uint32_t *__restrict__ tile_nproc, int n_tiles,
                                                       const int32_t *__restrict__ ranges,
                                                       const uint32_t *__restrict__ sorted_ids,
                                                       const uint4 *__restrict__ rects,
                                                       unsigned long long *__restrict__ stop_keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tiles) return;
    const uint32_t np = tile_nproc[i];
    uint32_t depth = 0, id = 0;
    if (np) {
        id = sorted_ids[(uint32_t)ranges[2 * i] + np - 1];
        depth = rects[id].z;
    }
    // two arrays of T words, depth bits first: the reader decides almost every pair from the 4-byte depth word alone (a
    // table of 32 KiB at 1080p instead of 64) and looks at the Gaussian index only where the depth bits are equal
    uint32_t *sk = reinterpret_cast<uint32_t *>(stop_keys);
    sk[i] = depth;
    sk[n_tiles + i] = id;
}

struct RefWs {
    uint32_t *tile_nproc, *bucket_offsets;
    uint4 *bucket_info;
    unsigned long long *n_buckets;
    float4 *ckpt;
    int64_t max_buckets;
    size_t bytes;
};
RefWs carve_ref(void *base, int64_t M, int32_t h, int32_t w) {
    RefWs r;
    const int n_tiles = (w / 16) * (h / 16);
    size_t off = 0;
    auto take = [&](size_t bytes) -> void * {
        void *p = base ? (void *)((char *)base + off) : nullptr;
        off += gs_align_up(bytes ? bytes : 1, 256);
        return p;
    };
    r.max_buckets = gs_max_buckets(M, n_tiles);
    r.tile_nproc = (uint32_t *)take(sizeof(uint32_t) * n_tiles);
    r.bucket_offsets = (uint32_t *)take(sizeof(uint32_t) * (n_tiles + 1));
    r.bucket_info = (uint4 *)take(sizeof(uint4) * (size_t)(r.max_buckets + 8));
    r.n_buckets = (unsigned long long *)take(sizeof(unsigned long long));
    r.ckpt = (float4 *)take(sizeof(float4) * 256 * (size_t)r.max_buckets);
    r.bytes = off;
    return r;
}

// The two parts of a frame's preparation that gs_stage_backward_prepare and gs_stage_contrib_prepare both issue.
// No row carries a flag: the readers decide from the tiles' stop keys which rows exist (rgb: round 4; SH: round 5 --
// until then a flag byte per pair, set by scattered one-byte stores = a 32-byte write each, cleared by a memset here)
void launch_stop_keys(const gs_frame_ws &ws, int n_tiles, const uint32_t *sorted_ids, hipStream_t stream) {
    hipLaunchKernelGGL(stop_key_kernel, dim3((unsigned)gs_div_up(n_tiles, 256)), dim3(256), 0, stream, ws.tile_nproc, n_tiles,
                       ws.tile_ranges, sorted_ids, ws.rects, (unsigned long long *)ws.stop_keys);
}
// ... and the frame's bucket work list, its count (and the saturated tiles' share) in *n_buckets
void launch_frame_bucket_list(const gs_frame_ws &ws, int n_tiles, unsigned long long *n_buckets, hipStream_t stream) {
    gs_launch_bucket_list(ws.tile_nproc, n_tiles, ws.bucket_offsets, n_buckets, ws.bucket_info, ws.tile_ranges, 1, stream);
}
// Which frames go to the matrix pipe: SH frames without maps.  Their preparation builds work items; every other frame --
// rgb, and GS_FRAME_AUX frames of every colour model -- takes a one-wave-per-bucket kernel and gets the bucket work list.
bool mfma_frame(const gs_frame *f) { return f->color_dim != 3 && !(f->flags & GS_FRAME_AUX); }

}  // namespace

extern "C" size_t gs_draw_backward_workspace_bytes(int64_t M, int32_t h, int32_t w) {
    if (M < 0 || h <= 0 || w <= 0) return 0;
    return carve_ref(nullptr, M, h, w).bytes;
}

extern "C" int gs_draw_backward(const float *pos, const float *rgb, const float *opa, const float *cov,
                                const int32_t *tile_n_point_accum, const float *output, const float *grad_output,
                                float *grad_pos, float *grad_rgb, float *grad_opa, float *grad_cov, int32_t h,
                                int32_t w, int64_t M, float focal_x, float focal_y, int weight_normalize,
                                int sigmoid, int fast, const float *rays_o, const float *lefttop_pos,
                                const float *vec_dx, const float *vec_dy, int use_sh_coeff, void *workspace,
                                size_t workspace_bytes, gs_stream_t stream) {
    const int exact = fast ? 0 : 1;  // fast = 0: the reference's exp() flavour (gaussian.cu:596-603, 922-923)
    (void)weight_normalize;  // the reference backward ignores it as well (gaussian.cu:440-803)
    GS_CHECK_ARG(h > 0 && w > 0 && (h % 16) == 0 && (w % 16) == 0, "h, w must be positive multiples of 16");
    GS_CHECK_ARG(M >= 0, "M < 0");
    if (M == 0) return 0;
    GS_CHECK_ARG(pos && rgb && opa && cov && tile_n_point_accum && output && grad_output && grad_pos && grad_rgb &&
                     grad_opa && grad_cov,
                 "null pointer");
    GS_CHECK_ARG(((uintptr_t)cov & 15) == 0 && ((uintptr_t)grad_cov & 15) == 0, "cov/grad_cov must be 16-byte aligned");
    GS_CHECK_ARG(workspace && workspace_bytes >= gs_draw_backward_workspace_bytes(M, h, w), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    RefWs ws = carve_ref(workspace, M, h, w);
    RasterSrc S;
    RasterGeom G;
    int rc = gs_ref_raster_args(__func__, pos, rgb, opa, cov, h, w, focal_x, focal_y, use_sh_coeff, rays_o, lefttop_pos, vec_dx,
                                vec_dy, S, G);
    if (rc) return rc;
    // 1. replay the forward to checkpoint (T, C_run) at every bucket boundary
    rc = gs_raster_forward_ref(S, G, tile_n_point_accum, nullptr, use_sh_coeff, sigmoid, 0, ws.ckpt, ws.tile_nproc, s, exact);
    if (rc) return rc;
    // 2. bucket work list
    gs_launch_bucket_list(ws.tile_nproc, G.ntx * G.nty, ws.bucket_offsets, ws.n_buckets, ws.bucket_info, tile_n_point_accum, 0, s);
    // 3. one wave per bucket, one output row per pair: the systolic kernel for `sigmoid`, the pixel-parallel one otherwise
    BwdIn I = {output, grad_output, ws.ckpt, ws.tile_nproc, ws.bucket_offsets, ws.bucket_info, tile_n_point_accum};
    BwdOut O = {nullptr, nullptr, nullptr, nullptr, 0, grad_pos, grad_rgb, grad_opa, grad_cov};  // (reference API: no rows)
    const int color_dim = use_sh_coeff ? 27 : 3;
    if (sigmoid)
        gs_launch_bwd_systolic(color_dim, exact, S, G, I, O, ws.max_buckets, s);
    else
        gs_launch_bwd_pixel(color_dim, false, exact, S, G, I, O, ws.max_buckets, s);
    GS_CHECK_LAUNCH();
    return 0;
}

// What the backward needs from the forward alone: which rows will exist -- rows of pairs behind a tile's
// early-termination point are never written, and the reader must skip them; the rows themselves, 64 to 224 bytes per
// pair, are not zero-filled (1.1 GB per frame at 2.4 M Gaussians with SH): one "stop key" per TILE -- and the work list:
// the bucket list the one-wave-per-bucket kernels read, or the work items the SH backward on the matrix pipe walks, heavy
// tiles first where the frame has an order.  gs_frame_forward runs it on a side stream underneath
// whatever the caller does between forward and backward (the loss); gs_frame_backward runs it inline otherwise.
int gs_stage_backward_prepare(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids, hipStream_t stream) {
    gs_frame_geom FG = gs_frame_geometry(f);
    launch_stop_keys(ws, FG.n_tiles, sorted_ids, stream);
    if (!mfma_frame(f))
        launch_frame_bucket_list(ws, FG.n_tiles, ws.counters + GS_CNT_BUCKETS, stream);
    else
        gs_launch_mfma_items(ws.tile_nproc, FG.n_tiles, (gs_frame_uses_strips(f) && f->N > 0) ? ws.tile_order : nullptr,
                             ws.mfma_items, ws.mfma_n_items, stream);
    GS_CHECK_LAUNCH();
    return 0;
}

// What gs_frame_contrib (contrib.hip) needs of the preparation above: the stop keys and the bucket work list.  `prepared`: the
// frame's own preparation has run or is queued in front of `stream`; then only SH frames without maps lack the list (they got
// work items instead), and theirs is built with its count in `n_buckets_own` -- nothing the backward of such a frame reads.
// Otherwise the launches of the preparation above: the list the backward will build again, bit for bit.
int gs_stage_contrib_prepare(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids, bool prepared,
                             unsigned long long *n_buckets_own, hipStream_t stream) {
    gs_frame_geom FG = gs_frame_geometry(f);
    if (!prepared) launch_stop_keys(ws, FG.n_tiles, sorted_ids, stream);
    if (mfma_frame(f))
        launch_frame_bucket_list(ws, FG.n_tiles, n_buckets_own, stream);
    else if (!prepared)
        launch_frame_bucket_list(ws, FG.n_tiles, ws.counters + GS_CNT_BUCKETS, stream);
    GS_CHECK_LAUNCH();
    return 0;
}

// The one place that decides which kernel a frame gets (the reference API's choice: gs_draw_backward above).
int gs_stage_raster_backward(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids,
                             const float *grad_image, hipStream_t stream, bool prepared) {
    RasterSrc S;
    RasterGeom G;
    gs_frame_raster_args(f, ws, sorted_ids, S, G);
    if (!prepared) {
        const int rc = gs_stage_backward_prepare(f, ws, sorted_ids, stream);
        if (rc) return rc;
    }
    BwdIn I = {f->image_padded, grad_image, ws.ckpt, ws.tile_nproc, ws.bucket_offsets, ws.bucket_info, ws.tile_ranges,
               (gs_frame_uses_strips(f) && f->N > 0) ? ws.tile_order : nullptr, 0u,
               (f->flags & GS_FRAME_BWD_ROWS) ? 1u : 0u, ws.mfma_items, ws.mfma_n_items};
    BwdOut O = {ws.rows, ws.bwd_exec_rows, ws.pair_offsets, ws.rects, (uint64_t)f->max_pairs, nullptr, nullptr, nullptr, nullptr};
    if (f->flags & GS_FRAME_AUX) {
        // every bucket of the work list on the pixel kernel with the depth / alpha terms, whatever the colour model
        const AuxBwdIn X = {(const float2 *)f->aux_padded, gs_frame_aux(f).ckpt, f->grad_depth, f->grad_alpha};
        gs_launch_bwd_aux(f->color_dim, S, G, I, O, X, ws.max_buckets, stream);
    } else if (mfma_frame(f))
        gs_launch_bwd_mfma(f->color_dim, S, G, I, O, ws.max_buckets, stream);
    else if (I.use_rows)
        gs_launch_bwd_rows(S, G, I, O, ws.max_buckets, stream);
    else
        gs_launch_bwd_pixel(3, true, 0, S, G, I, O, ws.max_buckets, stream);
    GS_CHECK_LAUNCH();
    // SH rows of Gaussians that cover hundreds of tiles are summed here, once, by whole workgroups (project_bwd.hip)
    return gs_stage_sh_big_rows(f, ws, stream);
}
