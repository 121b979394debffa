// contrib.hip -- per-Gaussian contribution statistics of a rendered training frame (gs_frame_contrib, include/gs_abi.h).
//
// The compositing weight w_g(p) = alpha_g(p) T_g(p) is formed in every forward and every backward and never leaves them per
// Gaussian.  Two launches let it out for a frame whose forward has run:
//   C1 contrib_pair_kernel     : one wave per bucket of the frame's work list (64 list entries of one tile, the transmittance
//                                of the tile's 256 pixels at the bucket's start in the forward's checkpoint).  The ROW layout of
//                                raster_backward_rows_kernel without its gradient algebra: lane = (Gaussian of a group of 16,
//                                pixel quad), a step is one pixel row of the tile, the transmittance in front of a Gaussian is a
//                                DPP row scan (gs_row_scan_mul4_excl, raster_common.h).  Sum, maximum and count over the
//                                tile's pixels accumulate in the lane's registers (a lane's pixels are its own: no cross-lane
//                                step inside the loop), the four quads of a Gaussian
//                                are combined once per group and one 16-byte pair row (sum, max, count, 0) goes to the slot the
//                                pair's gradient row has (emission order: pair_offsets[g] + the tile's index in g's rectangle).
//   C2 contrib_gaussian_kernel : a lane per Gaussian combines its rows that exist -- key(g) <= the tile's stop key, the reader's
//                                rule of project_bwd.hip; rows are never zero-filled -- in ascending row order and writes or
//                                accumulates its 16-byte row with one store.  A Gaussian with more than 64 rows has them loaded
//                                by its whole wave, 64 per round trip, and still added by its owner in ascending order: the same
//                                bits whichever way the rows arrive.
// No atomics; every sum runs in a fixed order (rows 0 .. 15 of the tile and the lane's four columns, then quads (0 + 1) + (2 +
// 3) in the butterfly's order; then rows ascending): bitwise repeatable whatever the workspace held.
// alpha and the masked transmittance are raster_backward_rows_kernel's expressions: alpha = 2^-(q + nlop) with the forward's
// evaluation order of q, T in front of a Gaussian = T at the bucket's start x the product of the earlier (1 - alpha), and
// alpha = 0 once that T has reached the 1e-4 stop.  Pixels of the padded border count for nothing.
#include <cmath>

#include "raster_bwd_common.h"  // bwd_frame_grid

namespace {

struct ContribIn {
    const float4 *ckpt;              // [max_buckets][256] (T, C) at bucket starts: the forward's checkpoints
    const uint32_t *bucket_offsets;  // [T + 1]
    const uint4 *bucket_info;        // (tile, first Gaussian, count, start of the tile's list) per bucket
    const uint32_t *pair_offsets;    // [N]
    const uint4 *rects;              // [N]
    uint64_t max_pairs;
};

// One wave per bucket, the work list walked with the grid as the stride (any grid is correct).
__global__ void __launch_bounds__(64) contrib_pair_kernel(RasterSrc S, RasterGeom G, ContribIn I, float w_min,
                                                         uint4 *__restrict__ pair_rows) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t NO_SLOT = 0xffffffffu;
    __shared__ __attribute__((aligned(16))) float s_T[256];  // transmittance in front of the current group
    __shared__ float s_py[16];
    auto lds_order = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    const int lane = threadIdx.x;
    const uint32_t gq = (uint32_t)lane & 15u, jq = (uint32_t)lane >> 4;  // Gaussian of the group, pixel quad
    const uint32_t n_tiles = (uint32_t)(G.ntx * G.nty), n_work = I.bucket_offsets[n_tiles];
    for (uint32_t kb = blockIdx.x; kb < n_work; kb += gridDim.x) {
        const uint4 info = I.bucket_info[kb];
        const uint32_t tile = info.x, base = info.y, r = info.z, start = info.w;
        const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
        const uint32_t id_lane = S.ids[start + base + ((uint32_t)lane < r ? (uint32_t)lane : r - 1)];
        {
            // the tile's pixels at the bucket's boundary: pixel 64 k + lane; the tile's first bucket starts from T = 1, which
            // the forward does not store (the slot read instead is a valid one of this tile: raster_ckpt_slot)
            const float4 *ck = I.ckpt + raster_ckpt_slot(start, tile, base / GS_BUCKET) * 256;
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = ck[64 * k + lane].x;
#pragma unroll
            for (int k = 0; k < 4; ++k) s_T[64 * k + lane] = base == 0 ? 1.f : t[k];
            if (lane < 16) s_py[lane] = raster_pixel_coord(ty * 16 + (uint32_t)lane, G.padH, G.focal_y);
        }
        float pxs[4];   // centres of this lane's four pixel columns
        bool col_in[4];  // ... and whether they lie inside the cropped image
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t id_x = tx * 16 + 4 * jq + i;
            pxs[i] = raster_pixel_coord(id_x, G.padW, G.focal_x);
            const int ox = (int)id_x - G.crop_left;
            col_in[i] = ox >= 0 && ox < G.width;
        }
        lds_order();

        const uint32_t ngrp = (r + 15) / 16;
        for (uint32_t grp = 0; grp < ngrp; ++grp) {
            // this lane's Gaussian (entries beyond r re-read the bucket's last one and are switched off: alpha = 0)
            const uint32_t gi = grp * 16 + gq;
            const bool valid = gi < r;
            const uint32_t gid = (uint32_t)__shfl((int)id_lane, (int)(valid ? gi : r - 1), 64);
            const float4 *rec = S.geom + (size_t)gid * GS_REC_STRIDE;  // one 64-byte line: geom | cov | colour | conic
            const float4 ge = rec[0], cq = rec[3];
            uint32_t slot = NO_SLOT;
            if (valid) {
                const uint4 rc = I.rects[gid];
                const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16;
                const uint64_t sl = (uint64_t)I.pair_offsets[gid] + (ty - y0) * (x1 - x0) + (tx - x0);
                if (sl < I.max_pairs) slot = (uint32_t)sl;
            }
            // alpha = sigma(opa) 2^-q = 2^-(q + nlop), nlop = -log2 sigma(opa), as the forward and the row-layout backward
            const float lopa = fmaxf(__log2f(ge.w), -200.0f);
            const float cC = cq.z, gy = ge.y;
            float nbdx[4], adx2[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dxi = pxs[i] - ge.x;
                nbdx[i] = -(cq.y * dxi);
                adx2[i] = valid ? fmaf(cq.x * dxi, dxi, -lopa) : 1e30f;  // (a padded entry: alpha = 0 exactly)
            }
            float wsum = 0.f, wmax = 0.f;
            uint32_t wcnt = 0;
#pragma unroll 2
            for (int s = 0; s < 16; ++s) {  // pixel row s of the tile
                const f4 T4 = *reinterpret_cast<const f4 *>(s_T + 16 * s + 4 * (int)jq);
                // a pixel row whose 16 pixels have all stopped has w = 0 for every Gaussian of the group, and its states
                // need not move (wave-uniform; the transmittance only falls)
                const bool any_live =
                    __ballot(T4[0] > GS_T_STOP || T4[1] > GS_T_STOP || T4[2] > GS_T_STOP || T4[3] > GS_T_STOP) != 0ull;
                if (!any_live) continue;
                const float dy = s_py[s] - gy;
                const int oy = (int)(ty * 16) + s - G.crop_top;
                const bool row_in = oy >= 0 && oy < G.height;  // (uniform)
                float araw[4], pin[4], Tb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float q = fmaf(fmaf(cC, dy, nbdx[i]), dy, adx2[i]);  // q + nlop, the forward's evaluation order
                    araw[i] = gs_exp2(-q);
                    pin[i] = fminf(fmaxf(1.0f - araw[i], 0.f), 1.0f);
                    Tb[i] = T4[i];
                }
                gs_row_scan_mul4_excl(pin, Tb);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float alpha = Tb[i] > GS_T_STOP ? araw[i] : 0.f;
                    const float w = (row_in && col_in[i]) ? alpha * Tb[i] : 0.f;
                    wsum += w;
                    wmax = fmaxf(wmax, w);
                    wcnt += w >= w_min ? 1u : 0u;
                }
                if (gq == 15) {  // the row's transmittance in front of the next group
                    f4 Tout;
#pragma unroll
                    for (int i = 0; i < 4; ++i) Tout[i] = T4[i] * pin[i];
                    *reinterpret_cast<f4 *>(s_T + 16 * s + 4 * (int)jq) = Tout;
                }
            }
            // the four pixel quads of the Gaussian: (0 + 1) + (2 + 3) in every lane alike
            wsum += __shfl_xor(wsum, 16, 64);
            wsum += __shfl_xor(wsum, 32, 64);
            wmax = fmaxf(wmax, __shfl_xor(wmax, 16, 64));
            wmax = fmaxf(wmax, __shfl_xor(wmax, 32, 64));
            wcnt += (uint32_t)__shfl_xor((int)wcnt, 16, 64);
            wcnt += (uint32_t)__shfl_xor((int)wcnt, 32, 64);
            if (jq == 0 && slot != NO_SLOT)
                pair_rows[slot] = make_uint4(__float_as_uint(wsum), __float_as_uint(wmax), wcnt, 0u);
            lds_order();  // (the next group reads the states the lanes of Gaussian 15 wrote)
        }
    }
}

// A lane per Gaussian.  rows_out[g] = (weight_sum, weight_max, pixels, views) of this frame, or what the buffer holds combined
// with it (accumulate).
constexpr uint32_t CONTRIB_BIG = 64;  // rows beyond which the wave loads a Gaussian's rows together
__global__ void __launch_bounds__(256) contrib_gaussian_kernel(const uint4 *__restrict__ rects,
                                                              const uint32_t *__restrict__ pair_offsets,
                                                              const float4 *__restrict__ rec_geom,
                                                              const unsigned long long *__restrict__ stop_keys,
                                                              const uint4 *__restrict__ pair_rows, uint32_t ntx,
                                                              uint32_t n_tiles, int cull_method, GsDistCull D, int64_t n,
                                                              uint64_t max_pairs, int accumulate,
                                                              uint4 *__restrict__ rows_out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = g < n;
    // (y0 | y1 << 16, x0 | x1 << 16, depth bits, tiles touched); depth bits != 0 <=> visible.  The rest of a culled Gaussian's
    // record is unspecified: not read
    const uint4 rc = valid ? rects[g] : make_uint4(0, 0, 0, 0);
    const bool vis = rc.z != 0;
    const uint32_t *stop_depth = reinterpret_cast<const uint32_t *>(stop_keys), *stop_id = stop_depth + n_tiles;
    const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16, bw = x1 - x0;
    const uint64_t off = vis ? pair_offsets[g] : 0;
    uint32_t cnt = vis && bw ? rc.w : 0u;
    if (off >= max_pairs) cnt = 0;
    else if (off + cnt > max_pairs) cnt = (uint32_t)(max_pairs - off);
    float cx = 0.f, cy = 0.f;
    if (cull_method == 0 && cnt) {  // "dist": not every tile of the bounding square is listed
        const float4 gg = rec_geom[g * GS_REC_STRIDE];
        cx = gg.x;
        cy = gg.y;
    }
    auto row_exists = [&](uint32_t dz, uint32_t id, uint32_t ix, uint32_t iy, float px, float py) {
        if (cull_method == 0 && !gs_dist_listed(px, py, ix, iy, D)) return false;
        const uint32_t t = iy * ntx + ix, sd = stop_depth[t];
        return dz < sd || (dz == sd && id <= stop_id[t]);
    };
    float wsum = 0.f, wmax = 0.f;
    uint32_t pix = 0;
    auto add_row = [&](const uint4 &v) {
        wsum += __uint_as_float(v.x);
        wmax = fmaxf(wmax, __uint_as_float(v.y));
        pix += v.z;
    };
    const bool big = cnt > CONTRIB_BIG;
    if (!big) {
        uint32_t ix = x0, iy = y0;
        for (uint32_t k = 0; k < cnt; ++k) {
            if (row_exists(rc.z, (uint32_t)g, ix, iy, cx, cy)) add_row(pair_rows[off + k]);
            if (++ix == x1) {
                ix = x0;
                ++iy;
            }
        }
    }
    // Gaussians that cover more than CONTRIB_BIG tiles, one after the other (uniform over the wave): lane l looks at row
    // k0 + l, the owner adds the window's rows in ascending order
    unsigned long long bm = __ballot(big);
    while (bm) {
        const int src = __ffsll((long long)bm) - 1;
        bm &= bm - 1;
        const uint32_t bz = (uint32_t)__shfl((int)rc.z, src, 64), bcnt = (uint32_t)__shfl((int)cnt, src, 64);
        const uint32_t bx0 = (uint32_t)__shfl((int)x0, src, 64), by0 = (uint32_t)__shfl((int)y0, src, 64);
        const uint32_t bbw = (uint32_t)__shfl((int)bw, src, 64);
        const uint32_t boff = (uint32_t)__shfl((int)(uint32_t)off, src, 64);
        const float bcx = __shfl(cx, src, 64), bcy = __shfl(cy, src, 64);
        const uint32_t bid = (uint32_t)(g - lane + src);
        for (uint32_t k0 = 0; k0 < bcnt; k0 += 64) {
            const uint32_t k = k0 + (uint32_t)lane;
            uint4 v = make_uint4(0, 0, 0, 0);
            bool ex = false;
            if (k < bcnt) {
                ex = row_exists(bz, bid, bx0 + k % bbw, by0 + k / bbw, bcx, bcy);
                if (ex) v = pair_rows[(uint64_t)boff + k];
            }
            unsigned long long m = __ballot(ex);
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                uint4 vj;
                vj.x = (uint32_t)__shfl((int)v.x, j, 64);
                vj.y = (uint32_t)__shfl((int)v.y, j, 64);
                vj.z = (uint32_t)__shfl((int)v.z, j, 64);
                vj.w = 0u;
                if (lane == src) add_row(vj);
            }
        }
    }
    if (!valid) return;
    uint4 o = make_uint4(__float_as_uint(wsum), __float_as_uint(wmax), pix, pix > 0 ? 1u : 0u);
    if (accumulate) {
        const uint4 h = rows_out[g];
        o.x = __float_as_uint(__uint_as_float(h.x) + wsum);
        o.y = __float_as_uint(fmaxf(__uint_as_float(h.y), wmax));
        o.z = h.z + pix;
        o.w = h.w + (pix > 0 ? 1u : 0u);
    }
    rows_out[g] = o;
}

constexpr size_t CONTRIB_HEADER = 256;  // the bucket count of a work list built here (8 bytes), line-aligned pair rows behind it

}  // namespace

size_t gs_contrib_workspace_bytes(int64_t max_pairs) {
    return CONTRIB_HEADER + gs_align_up(sizeof(uint4) * (size_t)(max_pairs > 0 ? max_pairs : 0), 256);
}

// The two launches (and what they need of the backward's preparation) for a validated training frame with N > 0.  `prepared`:
// the frame's own preparation is done or queued in front of `stream` (gs_frame.hip joins the side stream without consuming it).
int gs_stage_contrib(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids, bool prepared, float w_min,
                     int accumulate, gs_contrib_row *rows, void *workspace, hipStream_t stream) {
    gs_frame_geom FG = gs_frame_geometry(f);
    unsigned long long *n_own = (unsigned long long *)workspace;
    uint4 *pair_rows = (uint4 *)((char *)workspace + CONTRIB_HEADER);
    int rc = gs_stage_contrib_prepare(f, ws, sorted_ids, prepared, n_own, stream);
    if (rc) return rc;
    RasterSrc S;
    RasterGeom G;
    gs_frame_raster_args(f, ws, sorted_ids, S, G);
    const ContribIn I = {ws.ckpt, ws.bucket_offsets, ws.bucket_info, ws.pair_offsets, ws.rects, (uint64_t)f->max_pairs};
    // the grid of the one-wave-per-bucket backward kernels: the list's capacity, capped (the kernel strides over the list)
    hipLaunchKernelGGL(contrib_pair_kernel, dim3(bwd_frame_grid(ws.max_buckets)), dim3(64), 0, stream, S, G, I, w_min,
                       pair_rows);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(contrib_gaussian_kernel, dim3((unsigned)gs_div_up(f->N, 256)), dim3(256), 0, stream, ws.rects,
                       ws.pair_offsets, ws.rec_geom, (const unsigned long long *)ws.stop_keys, pair_rows, (uint32_t)FG.ntx,
                       (uint32_t)FG.n_tiles, (int)f->tile_culling_method, gs_frame_dist_cull(f), f->N, (uint64_t)f->max_pairs,
                       accumulate, reinterpret_cast<uint4 *>(rows));
    GS_CHECK_LAUNCH();
    return 0;
}
