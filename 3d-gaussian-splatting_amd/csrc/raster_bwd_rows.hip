// raster_bwd_rows.hip -- tile rasterizer backward, rgb frames flagged GS_FRAME_BWD_ROWS: lanes own Gaussians, a step is one
// pixel row of the tile.  The overview of the backward kernels and the gradient identities: raster_bwd.hip.
#include "raster_bwd_common.h"

namespace {

// rgb colours, frame path (round 5): the ROW layout of the SH kernel on the matrix pipe (raster_bwd_mfma.hip) without its
// matrix products.
//
// One wave per (tile, bucket of 64 Gaussians) -- the grid of raster_backward_pixel_sh_kernel<3>, which this kernel replaces in
// frames flagged GS_FRAME_BWD_ROWS --, but inside the bucket lanes own GAUSSIANS, not pixels: lane l = (Gaussian l & 15 of the current group of
// 16, pixel quad l >> 4), and a step is one pixel ROW of the tile: 16 Gaussians x 16 pixels, four (pixel, Gaussian) pairs per
// lane.  What that buys for rgb colours, where there is no contraction to hand to the matrix pipe:
//   * the ten per-Gaussian sums accumulate in the lane's registers over the 16 pixel rows (a lane's four pixel columns have
//     constant dx) and are reduced 4 : 1 once per group -- the pixel-parallel kernel reduces ten rows of 64 partials through
//     LDS for EVERY Gaussian (PMC round 4: 42.8 M LDS + ~40 M VALU wave instructions of its 237 M per launch);
//   * the Gaussian's constants live in registers (no nine broadcast LDS reads per Gaussian);
//   * a pixel row whose 16 pixels have all stopped is left out, wave-uniformly: 14 % of the row steps of the 2.4 M scene
//     (the pixel layout could only skip half tiles, 5 %, and lost the gain to the branches).
// What it pays: the transmittance / rho recursions over the group's 16 Gaussians are DPP row scans (36 DPP instructions per
// step against eight plain ones).  Two more savings that the SH kernel does not have yet: the opacity is folded into the
// exponent (alpha = 2^(log2 sigma(opa) - q), as the forward does: no G x opacity product; sum dL/dalpha G is (sum s) /
// sigma(opa) and sum s q is corrected by log2 sigma(opa) sum s at the group's end), and the transmittance in front of a
// Gaussian is ONE v_mul_f32_dpp (row_shr:1 of the scanned products times T_in, lanes without a source keep T_in).
// Rows leave as one aligned 64-byte line each, sixteen rows per store instruction; no flags (stop keys).  No atomics; the
// sums run in a fixed order: bitwise repeatable.
// This kernel in frames flagged GS_FRAME_BWD_ROWS (include/gs_abi.h: the caller's statistic says most buckets belong to
// saturated tiles), raster_backward_pixel_sh_kernel<3> in the others.
// Why not always: kernel traces on one box (profiles/r05_e_*) -- 2.4 M Gaussians, every tile saturates: 446 -> 408 us; 376 k
// Gaussians, none does and no row is ever left out: 276 -> 305 us (the DPP scans cost more than the LDS reduction they
// replace).  Why not per tile (built: two work lists, one kernel each): the second launch is serial behind the first on
// the stream and costs the tail of its slowest lone wave (33 us at 376 k Gaussians for the ~100 tiles that do saturate).
#ifndef GS_BWD_ROWS_WPE
#define GS_BWD_ROWS_WPE 4  // waves per SIMD the register allocation aims at
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GS_BWD_ROWS_WPE)))
raster_backward_rows_kernel(RasterSrc S, RasterGeom G, BwdIn I, BwdOut O) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr uint32_t GS_NO_SLOT = 0xffffffffu;
    constexpr int RW = gs_row_floats(3);
    __shared__ __attribute__((aligned(16))) float s_gr[3][256];  // dL/dC of the tile's pixels (masked: crop, clamp)
    __shared__ __attribute__((aligned(16))) float s_T[256];      // transmittance / rho in front of the current group
    __shared__ __attribute__((aligned(16))) float s_rho[256];
    __shared__ float s_py[16];
    auto lds_order = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    const int lane = threadIdx.x;
    const uint32_t gq = (uint32_t)lane & 15u, jq = (uint32_t)lane >> 4;  // Gaussian of the group, pixel quad
    // the work list with the grid as the stride: see raster_backward_pixel_sh_kernel
    const uint32_t n_tiles = (uint32_t)(G.ntx * G.nty), n_work = I.bucket_offsets[n_tiles];
    for (uint32_t kb = blockIdx.x; kb < n_work; kb += gridDim.x) {
    const uint4 info = I.bucket_info[kb];
    const uint32_t tile = info.x, base = info.y, r = info.z, start = info.w;
    const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
    // the bucket's 64 Gaussian ids, one per lane (a group learns its ids from a lane exchange)
    const uint32_t id_lane = S.ids[start + base + ((uint32_t)lane < r ? (uint32_t)lane : r - 1)];

    // ---- the tile's pixels at the bucket's boundary: pixel 64 k + lane = (x = lane & 15, y = (lane >> 4) + 4 k).  Every
    // load is issued before anything is waited for (see raster_backward_pixel_sh_body).
    {
        const uint32_t id_x = tx * 16 + ((uint32_t)lane & 15), id_y0 = ty * 16 + ((uint32_t)lane >> 4);
        const float4 *ck = I.ckpt + raster_ckpt_slot(start, tile, base / GS_BUCKET) * 256;
        float4 c[4];
        float f[4][3], gr[4][3];
        bool inside[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = ck[64 * k + lane];  // (stale for the tile's first bucket: replaced below)
            const uint32_t id_y = id_y0 + 4 * k;
            const float *cf = I.c_final + ((size_t)id_y * G.padW + id_x) * 3;
            const int ox = (int)id_x - G.crop_left, oy = (int)id_y - G.crop_top;
            inside[k] = ox >= 0 && ox < G.width && oy >= 0 && oy < G.height;
            const float *gp = I.grad + ((size_t)(inside[k] ? oy : 0) * G.width + (inside[k] ? ox : 0)) * 3;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                f[k][e] = cf[e];
                gr[k][e] = gp[e];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            asm volatile("" ::"v"(gr[k][0]), "v"(gr[k][1]), "v"(gr[k][2]), "v"(f[k][0]), "v"(f[k][1]), "v"(f[k][2]),
                         "v"(c[k].x), "v"(c[k].y), "v"(c[k].z), "v"(c[k].w));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = 64 * k + lane;
            float g3[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                g3[e] = (inside[k] && f[k][e] >= 0.f && f[k][e] <= 1.f) ? gr[k][e] : 0.f;
                s_gr[e][p] = g3[e];
            }
            // the tile's first bucket starts from the empty pixel (T, C) = (1, 0), which the forward does not store
            const float4 ci = base == 0 ? make_float4(1.f, 0.f, 0.f, 0.f) : c[k];
            s_T[p] = ci.x;
            // rho = dL/dC . (C_final - C_run): the only way the remaining colour enters dL/dalpha (gaussian.cu:716-722)
            s_rho[p] = g3[0] * (f[k][0] - ci.y) + g3[1] * (f[k][1] - ci.z) + g3[2] * (f[k][2] - ci.w);
        }
        if (lane < 16) s_py[lane] = raster_pixel_coord(ty * 16 + (uint32_t)lane, G.padH, G.focal_y);
    }
    float pxs[4];  // centres of this lane's four pixel columns
#pragma unroll
    for (int i = 0; i < 4; ++i) pxs[i] = raster_pixel_coord(tx * 16 + 4 * jq + i, G.padW, G.focal_x);
    lds_order();

    const uint32_t ngrp = (r + 15) / 16;
    for (uint32_t grp = 0; grp < ngrp; ++grp) {
        // ---- this lane's Gaussian (entries beyond r re-read the bucket's last one and are switched off: alpha = 0)
        const uint32_t gi = grp * 16 + gq;
        const bool valid = gi < r;
        const uint32_t gid = (uint32_t)__shfl((int)id_lane, (int)(valid ? gi : r - 1), 64);
        const float4 *rec = S.geom + (size_t)gid * GS_REC_STRIDE;  // ONE 64-byte line: geom | cov | colour | conic
        const float4 ge = rec[0], col = rec[2], cq = rec[3];
        uint32_t slot = GS_NO_SLOT;
        if (valid) {
            const uint4 rc = O.rects[gid];
            const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16;
            const uint64_t sl = (uint64_t)O.pair_offsets[gid] + (ty - y0) * (x1 - x0) + (tx - x0);
            if (sl < O.max_pairs) slot = (uint32_t)sl;
        }
        // alpha = sigma(opa) 2^-q = 2^-(q - log2 sigma(opa)): the opacity rides in the exponent's constant term (an opacity
        // that underflowed to 0 composites nothing: the clamp keeps q' finite, 2^-(q + 200) is flushed to 0)
        const float lopa = fmaxf(__log2f(ge.w), -200.0f);
        const float cC = cq.z, gy = ge.y, c0 = col.x, c1 = col.y, c2 = col.z;
        float nbdx[4], adx2[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dxi = pxs[i] - ge.x;
            nbdx[i] = -(cq.y * dxi);
            // (a padded entry: q' = 1e30 => alpha = 0 exactly, and 0 x 1e30 = 0 in the sum of s q')
            adx2[i] = valid ? fmaf(cq.x * dxi, dxi, -lopa) : 1e30f;
        }
        float Syy = 0.f;
        // The LDS operands of a pixel row are read where they are used: four resident waves per SIMD cover the LDS latency
        // (a request one row ahead measured equal and costs a second register set).
        struct RowIn {
            f4 T, R, G0, G1, G2;
            float py;
        };
        auto row_loads = [&](RowIn &d, int s) {
            const int prow = 16 * s + 4 * (int)jq;
            d.T = *reinterpret_cast<const f4 *>(s_T + prow);
            d.R = *reinterpret_cast<const f4 *>(s_rho + prow);
            d.G0 = *reinterpret_cast<const f4 *>(s_gr[0] + prow);
            d.G1 = *reinterpret_cast<const f4 *>(s_gr[1] + prow);
            d.G2 = *reinterpret_cast<const f4 *>(s_gr[2] + prow);
            d.py = s_py[s];
        };
        // The per-pixel algebra of a row step runs on PAIRS of the lane's four pixels (v_pk_fma_f32 / v_pk_mul_f32 /
        // v_pk_add_f32: two fp32 results per issue slot; the kernel sits at the VALU issue limit).  The DPP scans, the
        // exponentials / reciprocals and the stop-point selects stay per pixel.
        typedef float f2 __attribute__((ext_vector_type(2)));
        auto sp = [](float v) { return f2{v, v}; };
        auto pfma = [](f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); };
        f2 Scp[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, S1p[2] = {{0.f, 0.f}, {0.f, 0.f}}, Syp[2] = {{0.f, 0.f}, {0.f, 0.f}};
        f2 Sqp = {0.f, 0.f};
        const f2 nbdx2[2] = {{nbdx[0], nbdx[1]}, {nbdx[2], nbdx[3]}}, adx22[2] = {{adx2[0], adx2[1]}, {adx2[2], adx2[3]}};
        auto row_step = [&](int s) {  // pixel row s of the tile
            RowIn cur;
            row_loads(cur, s);
            // a pixel row whose 16 pixels have all stopped adds exact zeros to every sum of every Gaussian of the group and
            // its states need not move: left out (wave-uniform; the transmittance only falls)
            const bool any_live = __ballot(cur.T[0] > GS_T_STOP || cur.T[1] > GS_T_STOP || cur.T[2] > GS_T_STOP ||
                                           cur.T[3] > GS_T_STOP) != 0ull;
            if (!any_live) return;
            const float dy = cur.py - gy;
            const f2 dy2 = sp(dy);
            f2 q2[2];
            float araw[4], pin[4], Tb[4];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                q2[h] = pfma(pfma(sp(cC), dy2, nbdx2[h]), dy2, adx22[h]);  // q' = q - log2 sigma(opa); the forward's evaluation order
                araw[2 * h] = gs_exp2(-q2[h].x);
                araw[2 * h + 1] = gs_exp2(-q2[h].y);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (0 <= 1 - alpha <= 1 for sane records; as a clamp it is the subtraction's clamp modifier, and a NaN /
                // > 1 alpha of a broken record stops the pixel)
                pin[i] = fminf(fmaxf(1.0f - araw[i], 0.f), 1.0f);
                Tb[i] = cur.T[i];
            }
            // inclusive product over the group's Gaussians, in place; the transmittance in front of this Gaussian: T_in x the
            // product over the group's EARLIER Gaussians -- one DPP multiply: lane g >= 1 takes the scanned product of lane
            // g - 1, lane 0 has no source and keeps T_in
            gs_row_scan_mul4_excl(pin, Tb);
            float alpha[4], wg[4], ws[4];
            f2 w2[2], al2[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) alpha[i] = Tb[i] > GS_T_STOP ? araw[i] : 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                al2[h] = f2{alpha[2 * h], alpha[2 * h + 1]};
                w2[h] = al2[h] * f2{Tb[2 * h], Tb[2 * h + 1]};
                const f2 g0 = h ? cur.G0.zw : cur.G0.xy, g1 = h ? cur.G1.zw : cur.G1.xy, g2 = h ? cur.G2.zw : cur.G2.xy;
                const f2 wgh = w2[h] * pfma(g2, sp(c2), pfma(g1, sp(c1), g0 * sp(c0)));  // w (dL/dC . colour)
                wg[2 * h] = wgh.x;
                wg[2 * h + 1] = wgh.y;
            }
            // inclusive prefix sum of w gc over the group's Gaussians, OUT of place: the unscanned wg stays for s below
            gs_row_scan_add4_oop(ws, wg);
            f2 rho2[2], svs[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f2 R2 = h ? cur.R.zw : cur.R.xy;
                rho2[h] = R2 - f2{ws[2 * h], ws[2 * h + 1]};  // rho behind this Gaussian
                const f2 den = sp(1.00000011920928955f) - f2{araw[2 * h], araw[2 * h + 1]};
                const f2 beta = al2[h] * f2{gs_rcp(den.x), gs_rcp(den.y)};
                // s = dL/dalpha alpha with dL/dalpha = T gc - rho / (1 - alpha + 1e-7) (gaussian.cu:716-722)
                //   = w gc - rho beta,  beta = alpha / (1 - alpha + 1e-7): masked with alpha, like w
                const f2 sv = pfma(-rho2[h], beta, f2{wg[2 * h], wg[2 * h + 1]});
                const f2 g0 = h ? cur.G0.zw : cur.G0.xy, g1 = h ? cur.G1.zw : cur.G1.xy, g2 = h ? cur.G2.zw : cur.G2.xy;
                Scp[0] = pfma(g0, w2[h], Scp[0]);
                Scp[1] = pfma(g1, w2[h], Scp[1]);
                Scp[2] = pfma(g2, w2[h], Scp[2]);
                S1p[h] += sv;
                Syp[h] = pfma(sv, dy2, Syp[h]);
                svs[h] = sv;
                Sqp = pfma(sv, q2[h], Sqp);
            }
            const f2 ss = svs[0] + svs[1];
            Syy = fmaf((ss.x + ss.y) * dy, dy, Syy);
            if (gq == 15) {  // the row's pixel states in front of the next group: T behind the group's last Gaussian
                f4 Tout, Rout;
#pragma unroll
                for (int i = 0; i < 4; ++i) Tout[i] = cur.T[i] * pin[i];
                Rout.xy = rho2[0];
                Rout.zw = rho2[1];
                *reinterpret_cast<f4 *>(s_T + 16 * s + 4 * jq) = Tout;
                *reinterpret_cast<f4 *>(s_rho + 16 * s + 4 * jq) = Rout;
            }
        };
        for (int s = 0; s < 16; s += 2) {  // (two rows per trip: the shape the register allocation was tuned on)
            row_step(s);
            row_step(s + 1);
        }
        const float S1[4] = {S1p[0].x, S1p[0].y, S1p[1].x, S1p[1].y}, Sy[4] = {Syp[0].x, Syp[0].y, Syp[1].x, Syp[1].y};
        float Sc0 = Scp[0].x + Scp[0].y, Sc1 = Scp[1].x + Scp[1].y, Sc2 = Scp[2].x + Scp[2].y, Sq = Sqp.x + Sqp.y;
        // ---- close the group: the lane's four pixel columns, then the four pixel quads of the Gaussian
        const float4 cv = rec[1];
        float Sx = 0.f, Sxx = 0.f, Sxy = 0.f, Syt = 0.f, Stot = (S1[0] + S1[1]) + (S1[2] + S1[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dxi = pxs[i] - ge.x;
            const float sx = S1[i] * dxi;
            Sx += sx;
            Sxx = fmaf(sx, dxi, Sxx);
            Sxy = fmaf(Sy[i], dxi, Sxy);
            Syt += Sy[i];
        }
        auto quad_sum = [](float v) {
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            return v;
        };
        Sx = quad_sum(Sx);
        Syt = quad_sum(Syt);
        Sxx = quad_sum(Sxx);
        Sxy = quad_sum(Sxy);
        Syy = quad_sum(Syy);
        Sq = quad_sum(Sq);
        Stot = quad_sum(Stot);
        Sc0 = quad_sum(Sc0);
        Sc1 = quad_sum(Sc1);
        Sc2 = quad_sum(Sc2);
        // s = dL/dalpha alpha and alpha = G sigma(opa) on every live pixel: sum dL/dalpha G = (sum s) / sigma(opa); the
        // loop summed s q' with q' = q - log2 sigma(opa)
        const float Sopa = Stot * (ge.w > 0.f ? gs_rcp(ge.w) : 0.f);
        const float Su = fmaf(lopa, Stot, Sq) * GS_LN2;  // u = -ln G = q ln 2
        float piece[4];
        {
            const float a = cv.x, bb = cv.y, cc = cv.z, d = cv.w;
            const float iPn = 1.0f / (2.0f * raster_det(a, bb, cc, d) + 1e-14f);
            // every lane of the Gaussian holds the same sums: lane (g, jq) puts piece jq of the row together
            if (jq == 0) {
                piece[0] = GS_LN2 * (2.0f * cq.x * Sx - cq.y * Syt);
                piece[1] = GS_LN2 * (2.0f * cq.z * Syt - cq.y * Sx);
                piece[2] = iPn * (-Syy + 2.0f * d * Su);
                piece[3] = iPn * (Sxy - 2.0f * cc * Su);
            } else if (jq == 1) {
                piece[0] = iPn * (Sxy - 2.0f * bb * Su);
                piece[1] = iPn * (-Sxx + 2.0f * a * Su);
                piece[2] = Sopa;
                piece[3] = Sc0;
            } else {
                piece[0] = jq == 2 ? Sc1 : 0.f;
                piece[1] = jq == 2 ? Sc2 : 0.f;
                piece[2] = 0.f;
                piece[3] = 0.f;
            }
        }
        {
            // the group's 16 rows as ONE store instruction of whole 64-byte lines: destination lane 4 r + q takes piece q of
            // row r from lane (g = r, jq = q)
            const int dr = lane >> 2, dq = lane & 3, src = dr + 16 * dq;
            const uint32_t dslot = (uint32_t)__shfl((int)slot, dr, 64);
            float4 o;
            o.x = __shfl(piece[0], src, 64);
            o.y = __shfl(piece[1], src, 64);
            o.z = __shfl(piece[2], src, 64);
            o.w = __shfl(piece[3], src, 64);
            if (dslot != GS_NO_SLOT) reinterpret_cast<float4 *>(O.rows + (size_t)dslot * RW)[dq] = o;
        }
        lds_order();  // (the next group reads the states the lanes of Gaussian 15 wrote)
    }
    }  // work list
}

}  // namespace

// one wave per bucket on the capped grid: the kernel strides over the work list
void gs_launch_bwd_rows(const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O, int64_t max_buckets,
                        hipStream_t stream) {
    hipLaunchKernelGGL(raster_backward_rows_kernel, dim3(bwd_frame_grid(max_buckets)), dim3(64), 0, stream, S, G, I, O);
}
