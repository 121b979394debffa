// raster_bwd_pixel.hip -- tile rasterizer backward, lanes own pixels: every colour model of the reference API, rgb frames
// and, with the depth / alpha terms, every GS_FRAME_AUX frame.  The overview of the backward kernels and the gradient
// identities: raster_bwd.hip.
#include "raster_bwd_common.h"

namespace {

// The pixel-parallel bucket kernel, rgb and SH colours.  One wave per (tile, bucket of 64 Gaussians), lanes own four
// PIXELS (x, y0 + 4k: the forward's layout) as two packed pairs, the bucket's Gaussians are applied front to back from
// the bucket's checkpoint, dx and the Gaussian's constants are shared by the lane's four pixels.  What SH adds per
// (pixel, Gaussian):
//   colour_c = sigmoid(sum_k sh_k(pixel) coef[c][k])   (27 / 48 FMAs forward, packed over the pixel pair)
//   dL/dcoef[c][k] += dL/dC_c w colour_c (1 - colour_c) sh_k(pixel)   (27 / 48 sums over the tile's pixels)
// The basis values of the lane's four pixels live in registers for the whole bucket (9 or 16 pairs x 2), the
// coefficients of the current Gaussian are wave-uniform (read through the scalar cache), and the 7 + 27 (48) sums of
// a Gaussian are reduced over the wave through LDS: every lane adds NROW consecutive entries of the [NROW][64] array
// of partials, the lanes that own a row add the two or three slice sums that fall into it.  The colour and opacity
// sums go straight to the Gaussian's gradient row; the six geometry sums wait in LDS for the closing algebra.
// Why it replaces the systolic kernel for the frame path: that one spends ~125 VALU instructions per (pixel,
// Gaussian) step of ONE pixel per lane plus 25 % pipeline fill; here the per-pixel math is packed two pixels per
// instruction (v_pk_fma_f32 runs at the rate of v_fma_f32 on this chip: tools/ubench/sort_ops.hip), dx and the
// Gaussian's constants are shared by the lane's four pixels and there is no fill: ~400 instructions per Gaussian
// per wave = 1.6 per (pixel, Gaussian) against 2.4.
template <int CDIM>
struct PixShCfg {
    static constexpr int NB = CDIM > 3 ? CDIM / 3 : 1;
    static constexpr int NROW = 7 + CDIM;  // Sx Sy Sxx Sxy Syy Sq Sopa + the colour(-coefficient) sums
};

#ifndef GS_BWD_SH48_WPE
#define GS_BWD_SH48_WPE 3
#endif
#ifndef GS_BWD_SH_WPE
#define GS_BWD_SH_WPE 4  // waves per SIMD the register allocation aims at (tunable, tools/ab_variants.py)
#endif

// The body of the pixel-parallel backward.  AUX = true: the maps are two more "colour channels" d_i and 1 -- dL/dalpha_i gains
// g_D (d_i T - (D_final - D_<=i) / (1 - alpha)) + g_A (T - (A_final - A_<=i) / (1 - alpha)) through the same gc / rho recursion,
// and one more row sum, sum_pixels g_D w_i = dL/dd_i, goes into the pair's row (gs_row_aux_depth).  AUX = false compiles to
// the plain kernel unchanged.
template <int CDIM, bool FRAME, bool EXACT, bool AUX>
__device__ __forceinline__ void raster_backward_pixel_sh_body(RasterSrc S, RasterGeom G, BwdIn I, BwdOut O,
                                                              const AuxBwdIn &X) {
    static_assert(!(EXACT && FRAME), "the exact-exp flavour belongs to the reference API (gs_draw_backward, fast = 0)");
    static_assert(!AUX || (FRAME && !EXACT), "depth / alpha maps belong to the frame path");
    constexpr int NB = PixShCfg<CDIM>::NB, NROW0 = PixShCfg<CDIM>::NROW;
    constexpr int NROW = NROW0 + (AUX ? 1 : 0);  // AUX: row NROW0 = sum g_D w (the depth gradient)
    constexpr bool PRE = CDIM == 27;  // degree 2: SH basis pre-scaled by -log2(e): raster_common.h
    typedef float f2 __attribute__((ext_vector_type(2)));
    enum { FX, FY, FA, FB, FC, FOPA, FC0, FC1, FC2, NFLD };  // FC0..2: the Gaussian's colour (CDIM == 3 only)
    __shared__ float s_g[NFLD][64];
    __shared__ uint32_t s_id[64];          // FRAME: Gaussian id; else index of the pair in the sorted arrays
    __shared__ float s_dep[AUX ? 64 : 1];  // AUX: d_i = rec_geom.z
    // [row][lane] partial sums of the current Gaussian, 16 rows at a time (rows padded to 65).  rgb colours have only 10
    // rows: 2.6 instead of 4.2 KiB, 7.6 KiB of LDS per wave in all -- five resident waves per SIMD instead of four
    // (same-box A/B, round 3: 0.377 -> 0.359 ms at cfg2, 0.547 -> 0.515 ms at 2.4 M Gaussians)
    __shared__ float s_red[(NROW < 16 ? NROW : 16) * 65];
    __shared__ float s_part[NROW][4];      // quarter-row sums of the first reduction level
    // geometry sums per Gaussian (Sx Sy Sxx Sxy Syy Sq).  rgb frame rows: also the opacity and the three colour sums --
    // the complete 10-float row is put together here and leaves as ONE aligned 64-byte line at the end of the bucket
    // (four lanes x 16 bytes).  Round 3 stored floats 6..9 of a row from the Gaussian loop and the geometry part after
    // it: two or three partial 32-byte sectors per 48-byte row plus a flag byte = 134 bytes of HBM writes per row.
    constexpr bool STAGED = FRAME && CDIM == 3;
    constexpr int TOTW = STAGED ? (AUX ? 11 : 10) : 8;
    __shared__ float s_tot[64][TOTW];
    __shared__ uint32_t s_slot[64];        // FRAME: emission slot of Gaussian i's gradient row (GS_NO_SLOT: no row)
    constexpr uint32_t GS_NO_SLOT = 0xffffffffu;
    auto lds_order = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    const int lane = threadIdx.x & 63;
    // The work list is walked with the grid as the stride (round 5): the launch need not cover the list's CAPACITY
    // (max_pairs / 64 + T buckets: 128 k waves at 2.4 M Gaussians, of which 31 k have a bucket -- the empty ones cost the
    // dispatcher 22 us of the kernel's 455, kernel trace profiles/r05_d_*), any grid is correct, and a grid beyond the
    // list's length gives every wave at most one bucket, as before (gs_launch_bwd_pixel picks it).
    const uint32_t n_tiles = (uint32_t)(G.ntx * G.nty), n_work = I.bucket_offsets[n_tiles];
    for (uint32_t kb = blockIdx.x; kb < n_work; kb += gridDim.x) {
    const uint4 info = I.bucket_info[kb];
    const uint32_t tile = info.x, base = info.y, r = info.z, start = info.w;
    if (base < I.skip_buckets * GS_BUCKET) continue;  // (uniform; never taken: see BwdIn)
    const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;

    // ---- this lane's Gaussian (lanes >= r re-read the bucket's last one and are zeroed below)
    GaussianRec g;
    const uint32_t jl = start + base + ((uint32_t)lane < r ? (uint32_t)lane : r - 1);
    const uint32_t gid = raster_load<FRAME>(S, jl, g);
    const uint32_t id_x = tx * 16 + (lane & 15), id_y0 = ty * 16 + (lane >> 4);
    const float px = raster_pixel_coord(id_x, G.padW, G.focal_x);
    const float4 *ck = I.ckpt + raster_ckpt_slot(start, tile, base / GS_BUCKET) * 256;
    float4 c[4];
    float f[4][3], gr[4][3];
    bool inside[4];
    float2 xfin[4], xck[4];  // AUX: final (D, A) and (D, A) at the bucket's start
    float xgd[4], xga[4];    // AUX: dL/dD, dL/dA
    (void)xfin; (void)xck; (void)xgd; (void)xga;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = ck[64 * k + lane];
        if constexpr (AUX) {
            const uint32_t id_y = id_y0 + 4 * k;
            xfin[k] = X.padded[(size_t)id_y * G.padW + id_x];
            xck[k] = base == 0 ? make_float2(0.f, 0.f) : X.ckpt[raster_ckpt_slot(start, tile, base / GS_BUCKET) * 256 + 64 * k + lane];
            const int ox = (int)id_x - G.crop_left, oy = (int)id_y - G.crop_top;
            const bool in = ox >= 0 && ox < G.width && oy >= 0 && oy < G.height;
            const size_t pi = (size_t)(in ? oy : 0) * G.width + (in ? ox : 0);
            xgd[k] = (in && X.grad_depth) ? X.grad_depth[pi] : 0.f;
            xga[k] = (in && X.grad_alpha) ? X.grad_alpha[pi] : 0.f;
        }
        const uint32_t id_y = id_y0 + 4 * k;
        const float *cf = I.c_final + ((size_t)id_y * G.padW + id_x) * 3;
        const int ox = FRAME ? (int)id_x - G.crop_left : (int)id_x, oy = FRAME ? (int)id_y - G.crop_top : (int)id_y;
        inside[k] = !FRAME || (ox >= 0 && ox < G.width && oy >= 0 && oy < G.height);
        const float *gp = I.grad + ((size_t)(inside[k] ? oy : 0) * (FRAME ? G.width : G.padW) + (inside[k] ? ox : 0)) * 3;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            f[k][e] = cf[e];
            gr[k][e] = gp[e];
        }
    }
    // the compiler would otherwise sink each gradient load behind its `inside` test and wait for it there: four
    // dependent round trips instead of one
#pragma unroll
    for (int k = 0; k < 4; ++k)
        asm volatile("" ::"v"(gr[k][0]), "v"(gr[k][1]), "v"(gr[k][2]), "v"(f[k][0]), "v"(f[k][1]), "v"(f[k][2]),
                     "v"(c[k].x), "v"(c[k].y), "v"(c[k].z), "v"(c[k].w));
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 3; ++e)
            gr[k][e] = (inside[k] && (!FRAME || (f[k][e] >= 0.f && f[k][e] <= 1.f))) ? gr[k][e] : 0.f;
    float cA = 0, cB = 0, cC = 0;
    {
        const bool valid = (uint32_t)lane < r;
        raster_conic(g, cA, cB, cC);
        s_g[FX][lane] = g.x;
        s_g[FY][lane] = g.y;
        s_g[FA][lane] = cA;
        s_g[FB][lane] = cB;
        s_g[FC][lane] = cC;
        s_g[FOPA][lane] = valid ? g.opa : 0.f;  // opacity 0 => alpha 0: padded entries contribute exact zeros
        if (CDIM == 3) {
            float r0, r1, r2;
            raster_load_rgb<FRAME>(S, jl, gid, r0, r1, r2);
            s_g[FC0][lane] = r0;
            s_g[FC1][lane] = r1;
            s_g[FC2][lane] = r2;
        }
        s_id[lane] = FRAME ? gid : jl;
        if constexpr (AUX) s_dep[lane] = S.geom[(size_t)gid * GS_REC_STRIDE].z;
        uint32_t myslot = GS_NO_SLOT;
        if (valid && FRAME) {
            const uint4 rc = O.rects[gid];
            const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16;
            const uint64_t slot = (uint64_t)O.pair_offsets[gid] + (ty - y0) * (x1 - x0) + (tx - x0);
            // (no flag per row: the reader derives "written" from the tile's stop key, gs_frame_layout.h; SH rows: every
            // float of the row is written below -- coefficients, geometry, padding)
            if (slot < O.max_pairs) myslot = (uint32_t)slot;  // (max_pairs < 2^30: gs_frame validate)
        }
        s_slot[lane] = myslot;
    }
    // pixel pairs: h = 0: rows y0, y0 + 4 (k = 0, 1); h = 1: rows y0 + 8, y0 + 12 (k = 2, 3)
    f2 py2[2], T[2], rho[2], g0[2], g1[2], g2[2], SHB[2][NB];
    f2 gD[AUX ? 2 : 1], gA[AUX ? 2 : 1];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (CDIM > 3) {
            float sa[NB], sb[NB];
            raster_pixel_sh<NB>(id_x, id_y0 + 8 * h, G, sa);
            raster_pixel_sh<NB>(id_x, id_y0 + 8 * h + 4, G, sb);
            // pre-scaled by -log2(e) (raster_common.h): the colour's exponent needs no multiplication, and the same
            // registers serve the coefficient gradients, whose factor c (1 - c) is scaled by -ln 2 instead (below)
            // (not at degree 3: there the kernel sits at its register limit and the change costs four more spilled
            // registers -- measured 2.22 against 2.12 ms; degree 2: 1.60 against 1.62 ms)
            constexpr float KS = PRE ? -GS_LOG2E : 1.0f;
#pragma unroll
            for (int k = 0; k < NB; ++k) SHB[h][k] = f2{KS * sa[k], KS * sb[k]};
        }
        py2[h] = f2{raster_pixel_coord(id_y0 + 8 * h, G.padH, G.focal_y),
                    raster_pixel_coord(id_y0 + 8 * h + 4, G.padH, G.focal_y)};
        float Tk[2], rk[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = 2 * h + e;
            // the tile's first bucket starts from the empty pixel (T, C) = (1, 0), which the forward does not store
            const float4 ci = base == 0 ? make_float4(1.f, 0.f, 0.f, 0.f) : c[k];
            Tk[e] = ci.x;
            rk[e] = gr[k][0] * (f[k][0] - ci.y) + gr[k][1] * (f[k][1] - ci.z) + gr[k][2] * (f[k][2] - ci.w);
            if constexpr (AUX)  // the maps' suffixes behind the bucket's start
                rk[e] += xgd[k] * (xfin[k].x - xck[k].x) + xga[k] * (xfin[k].y - xck[k].y);
        }
        if constexpr (AUX) {
            gD[h] = f2{xgd[2 * h], xgd[2 * h + 1]};
            gA[h] = f2{xga[2 * h], xga[2 * h + 1]};
        }
        T[h] = f2{Tk[0], Tk[1]};
        rho[h] = f2{rk[0], rk[1]};
        g0[h] = f2{gr[2 * h][0], gr[2 * h + 1][0]};
        g1[h] = f2{gr[2 * h][1], gr[2 * h + 1][1]};
        g2[h] = f2{gr[2 * h][2], gr[2 * h + 1][2]};
    }
    lds_order();

    auto splat = [](float v) { return f2{v, v}; };
    auto pk_fma = [](f2 a, f2 b, f2 cc) { return __builtin_elementwise_fma(a, b, cc); };
    // first reduction level: in round rd this lane adds quarter `lane / 16` (16 consecutive entries) of row
    // 16 rd + lane % 16 -- with rows padded to 65 floats the 64 lanes of a read hit every LDS bank exactly twice
    constexpr int NROUND = (NROW + 15) / 16;
    const uint32_t red_row = (uint32_t)lane & 15, red_part = (uint32_t)lane >> 4;

    // the coefficients of Gaussian i sit at a wave-uniform address (one cache line broadcast to the wave); those of
    // Gaussian i + 1 are requested as soon as the forward evaluation of Gaussian i has consumed the registers, so
    // that the round trip hides behind the gradient half of the iteration
    float co[CDIM];
    auto load_coef = [&](uint32_t i) {
        const uint32_t id = __builtin_amdgcn_readfirstlane(s_id[i]);
        if constexpr (CDIM > 3) {
            const float *cf = (FRAME ? S.sh : S.rgb) + (size_t)id * CDIM;
#pragma unroll
            for (int k = 0; k < CDIM; ++k) co[k] = cf[k];
        }
        return id;
    };
    uint32_t id_next = load_coef(0);
    constexpr bool PAIR_SKIP = CDIM == 27;  // the finished-half-tile skip: degree-2 SH only (below)
    bool pair_live[2] = {true, true};
    (void)pair_live;
    for (uint32_t i = 0; i < r; ++i) {
        const float gx = s_g[FX][i], gy = s_g[FY][i], uA = s_g[FA][i], uB = s_g[FB][i], uC = s_g[FC][i];
        const float opa = s_g[FOPA][i];
        const uint32_t id_i = id_next;
        const float dx = px - gx;
        const float bdx = uB * dx, adx2 = uA * dx * dx;
        f2 S1 = {0.f, 0.f}, Sy = S1, Syy = S1, Sq = S1, Sopa = S1, Sd = S1;
        const float dep_i = AUX ? s_dep[i] : 0.f;
        (void)dep_i;
        f2 D[2][3];
        // A pixel pair (= a half of the tile: rows 8 h .. 8 h + 7) whose 128 pixels are all finished adds exact zeros to
        // every sum below and its transmittance no longer changes: it is left out (wave-uniform branch, re-evaluated
        // every 8 Gaussians; the transmittance only falls, so a finished pair stays finished).  5 % of the pair
        // evaluations of the 2.4 M scene (oracle statistics).  Degree-2 SH only -- same-box A/B at 2.4 M
        // Gaussians: 1.40 -> 1.34 ms; degree 3 is at its register limit and loses (2.13 -> 2.42 ms: 18 spills), rgb
        // colours have too little work per pair to pay for the branches (0.63 = 0.63 ms, cfg2 +4 %).
        if constexpr (PAIR_SKIP) {
            if ((i & 7u) == 0) {
#pragma unroll
                for (int h = 0; h < 2; ++h) pair_live[h] = __ballot(T[h].x > GS_T_STOP || T[h].y > GS_T_STOP) != 0ull;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (PAIR_SKIP) {
                if (!pair_live[h]) {  // uniform
                    D[h][0] = D[h][1] = D[h][2] = f2{0.f, 0.f};
                    continue;
                }
            }
            const f2 dy = py2[h] - splat(gy);
            const f2 q = pk_fma(pk_fma(splat(uC), dy, splat(-bdx)), dy, splat(adx2));
            // EXACT: a double-precision exp of the float argument, as the reference's backward does for fast = 0
            // (gaussian.cu:596-603)
            const f2 Gv = EXACT ? f2{(float)exp(-(double)(q.x * GS_LN2)), (float)exp(-(double)(q.y * GS_LN2))}
                                : f2{gs_exp2(-q.x), gs_exp2(-q.y)};
            // colours of the pixel pair
            f2 c0, c1, c2;
            if constexpr (CDIM > 3) {
                f2 v0 = {0.f, 0.f}, v1 = v0, v2 = v0;
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    v0 = pk_fma(SHB[h][k], splat(co[k]), v0);
                    v1 = pk_fma(SHB[h][k], splat(co[NB + k]), v1);
                    v2 = pk_fma(SHB[h][k], splat(co[2 * NB + k]), v2);
                }
                auto sg = [](float v) { return PRE ? gs_rcp(1.0f + gs_exp2(v)) : gs_rcp(1.0f + __expf(-v)); };
                c0 = f2{sg(v0.x), sg(v0.y)};
                c1 = f2{sg(v1.x), sg(v1.y)};
                c2 = f2{sg(v2.x), sg(v2.y)};
            } else {  // one colour per Gaussian
                c0 = splat(s_g[FC0][i]);
                c1 = splat(s_g[FC1][i]);
                c2 = splat(s_g[FC2][i]);
            }
            // 1 / (1 - alpha + 1e-7) (gaussian.cu:722) as ONE fma + rcp: the constant is the fp32 neighbour of
            // 1 + 1e-7 (1 + 2^-23), 2e-8 away -- below the rounding of the two-step form it replaces
            const f2 den = pk_fma(-Gv, splat(opa), splat(1.00000011920928955f));
            const f2 rc = {gs_rcp(den.x), gs_rcp(den.y)};
            const bool l0 = T[h].x > GS_T_STOP, l1 = T[h].y > GS_T_STOP;
            const f2 araw = Gv * splat(opa);
            const f2 alpha = {l0 ? araw.x : 0.f, l1 ? araw.y : 0.f};
            const f2 w = alpha * T[h];
            f2 gc = pk_fma(g2[h], c2, pk_fma(g1[h], c1, g0[h] * c0));
            if constexpr (AUX) {
                gc += pk_fma(gD[h], splat(dep_i), gA[h]);  // the two maps as colour channels d_i and 1
                Sd = pk_fma(gD[h], w, Sd);
            }
            rho[h] = pk_fma(-w, gc, rho[h]);
            f2 d_alpha = pk_fma(T[h], gc, -(rho[h] * rc));
            d_alpha = f2{l0 ? d_alpha.x : 0.f, l1 ? d_alpha.y : 0.f};
            if constexpr (CDIM > 3) {
                // c (1 - c) [x -ln 2 with the pre-scaled basis: D sh' = D sh] as c (K - K c): one packed FMA either way
                constexpr float K = PRE ? -GS_LN2 : 1.0f;
                const f2 kk = {K, K}, nk = {-K, -K};
                D[h][0] = g0[h] * w * (c0 * pk_fma(c0, nk, kk));
                D[h][1] = g1[h] * w * (c1 * pk_fma(c1, nk, kk));
                D[h][2] = g2[h] * w * (c2 * pk_fma(c2, nk, kk));
            } else {  // dL/dcolour_c = sum dL/dC_c w (the sigmoid's derivative is applied per Gaussian, later)
                D[h][0] = g0[h] * w;
                D[h][1] = g1[h] * w;
                D[h][2] = g2[h] * w;
            }
            Sopa = pk_fma(d_alpha, Gv, Sopa);
            const f2 s = d_alpha * alpha;
            const f2 sdy = s * dy;
            S1 += s;
            Sy += sdy;
            Syy = pk_fma(sdy, dy, Syy);
            Sq = pk_fma(s, q, Sq);
            T[h] = T[h] - w;
        }
        id_next = load_coef(i + 1 < r ? i + 1 : i);
        // row m of the [NROW][64] array of partial sums: 0..6 geometry / opacity, 7 + ch NB + k colour (coefficient)
        const float s1 = S1.x + S1.y, sy_ = Sy.x + Sy.y;
        const float sx_ = s1 * dx;
        auto row_value = [&](int m) -> float {
            if (m == 0) return sx_;                // Sx
            if (m == 1) return sy_;                // Sy
            if (m == 2) return sx_ * dx;           // Sxx
            if (m == 3) return sy_ * dx;           // Sxy
            if (m == 4) return Syy.x + Syy.y;      // Syy
            if (m == 5) return Sq.x + Sq.y;        // Sq
            if (m == 6) return Sopa.x + Sopa.y;
            if (AUX && m == NROW0) return Sd.x + Sd.y;
            const int ch = (m - 7) / NB, k = (m - 7) % NB;
            if constexpr (CDIM > 3) {
                // four products of the lane's four pixels as ONE chain of scalar FMAs: a packed multiply + packed FMA +
                // the add of the two halves is three instructions but 5.2 ns of issue (packed fp32 has no rate
                // advantage on this chip: tools/ubench/pk_rate.hip), the chain is four instructions and 4.2 ns
                return fmaf(D[1][ch].y, SHB[1][k].y,
                            fmaf(D[1][ch].x, SHB[1][k].x, fmaf(D[0][ch].y, SHB[0][k].y, D[0][ch].x * SHB[0][k].x)));
            } else {
                const f2 p = D[0][ch] + D[1][ch];
                return p.x + p.y;
            }
        };
        // 16 rows at a time through a [16][65] window: the whole [NROW][65] array (8.8 / 14.3 KiB per wave) capped the
        // kernel at 2-3 waves per SIMD
#pragma unroll
        for (int rd = 0; rd < NROUND; ++rd) {
#pragma unroll
            for (int m = 16 * rd; m < 16 * rd + 16 && m < NROW; ++m) s_red[(m - 16 * rd) * 65 + lane] = row_value(m);
            lds_order();
            const uint32_t row = 16 * rd + red_row;
            if (16 * (rd + 1) <= NROW || row < (uint32_t)NROW) {
                const float *src = s_red + red_row * 65 + red_part * 16;
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                for (int j = 0; j < 16; j += 4) {
                    a0 += src[j];
                    a1 += src[j + 1];
                    a2 += src[j + 2];
                    a3 += src[j + 3];
                }
                s_part[row][red_part] = (a0 + a1) + (a2 + a3);
            }
            lds_order();
        }
        if (lane < NROW) {
            const float t = (s_part[lane][0] + s_part[lane][1]) + (s_part[lane][2] + s_part[lane][3]);
            if (lane < 6 || STAGED) {
                s_tot[i][lane] = t;
            } else if (FRAME) {
                const uint32_t sl = s_slot[i];  // sum dL/dalpha G (opacity), then the coefficient sums (row layout: gs_frame_layout.h)
                if (sl != GS_NO_SLOT)
                    O.rows[(size_t)sl * gs_row_floats(CDIM) +
                           (lane == 6                  ? gs_row_geo(CDIM, 6)
                            : (AUX && lane == NROW0) ? gs_row_aux_depth(CDIM)
                                                     : gs_row_col(CDIM, lane - 7))] = t;
            } else {
                const size_t j = id_i;
                if (lane == 6)
                    O.grad_opa[j] = t;
                else
                    O.grad_rgb[j * CDIM + (lane - 7)] = t;
            }
        }
        lds_order();
    }
    if ((uint32_t)lane < r) {  // one lane per Gaussian finishes the geometry algebra
        const float *t = s_tot[lane];
        const float Sx = t[0], Sy = t[1], Sxx = t[2], Sxy = t[3], Syy = t[4], Sq = t[5];
        const float a = g.a, b = g.b, cc = g.c, d = g.d;
        const float iPn = 1.0f / (2.0f * raster_det(a, b, cc, d) + 1e-14f);
        const float Su = Sq * GS_LN2;
        const float ogx = GS_LN2 * (2.0f * cA * Sx - cB * Sy), ogy = GS_LN2 * (2.0f * cC * Sy - cB * Sx);
        const float ga = iPn * (-Syy + 2.0f * d * Su), gb = iPn * (Sxy - 2.0f * cc * Su);
        const float gcc = iPn * (Sxy - 2.0f * b * Su), gd = iPn * (-Sxx + 2.0f * a * Su);
        if (STAGED) {  // the finished geometry part replaces the sums it was computed from (this lane's own entries)
            float *t2 = s_tot[lane];
            t2[0] = ogx; t2[1] = ogy; t2[2] = ga; t2[3] = gb; t2[4] = gcc; t2[5] = gd;
        } else if (FRAME) {
            const uint32_t sl = s_slot[lane];
            if (sl != GS_NO_SLOT) {
                constexpr int RW = gs_row_floats(CDIM);
                float *row = O.rows + (size_t)sl * RW;
                reinterpret_cast<float4 *>(row + gs_row_geo(CDIM, 0))[0] = make_float4(ogx, ogy, ga, gb);
                reinterpret_cast<float2 *>(row + gs_row_geo(CDIM, 4))[0] = make_float2(gcc, gd);
                // the floats of the row that are neither a sum nor the geometry: zero (the reader adds whole rows)
#pragma unroll
                for (int m = 0; m < RW; ++m) {
                    bool used = false;
#pragma unroll
                    for (int e = 0; e < 7; ++e) used = used || m == gs_row_geo(CDIM, e);
#pragma unroll
                    for (int e = 0; e < CDIM; ++e) used = used || m == gs_row_col(CDIM, e);
                    if (AUX) used = used || m == gs_row_aux_depth(CDIM);
                    if (!used) row[m] = 0.f;
                }
            }
        } else {
            const size_t j = (size_t)start + base + lane;
            O.grad_pos[j * 3 + 0] = ogx;
            O.grad_pos[j * 3 + 1] = ogy;
            reinterpret_cast<float4 *>(O.grad_cov)[j] = make_float4(ga, gb, gcc, gd);
        }
    }
    if constexpr (STAGED) {
        // rows leave as whole 64-byte lines: lane l stores quarter l % 4 of row 16 it + l / 4 -- sixteen rows per store
        // instruction, every line written completely by one instruction (floats 10..15 are zero padding)
        lds_order();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const uint32_t j = 16u * it + ((uint32_t)lane >> 2), qd = (uint32_t)lane & 3u;
            if (j >= r) break;  // (lanes of one row leave together; rows beyond r do not exist)
            const uint32_t sl = s_slot[j];
            if (sl == GS_NO_SLOT) continue;
            const float *t = s_tot[j];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qd == 0) v = make_float4(t[0], t[1], t[2], t[3]);
            else if (qd == 1) v = make_float4(t[4], t[5], t[6], t[7]);
            else if (qd == 2) v = make_float4(t[8], t[9], AUX ? t[TOTW - 1] : 0.f, 0.f);  // (AUX: float 10 = the depth sum)
            reinterpret_cast<float4 *>(O.rows + (size_t)sl * gs_row_floats(3))[qd] = v;
        }
    }
    lds_order();  // (the next bucket of this wave reuses the LDS arrays)
    }
}

template <int CDIM, bool FRAME, bool EXACT = false>
__global__ void __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(CDIM == 48 ? GS_BWD_SH48_WPE : CDIM == 3 ? 5 : GS_BWD_SH_WPE)))  // rgb: five (LDS: 7.9 KiB per wave)
raster_backward_pixel_sh_kernel(RasterSrc S, RasterGeom G, BwdIn I, BwdOut O) {
    raster_backward_pixel_sh_body<CDIM, FRAME, EXACT, false>(S, G, I, O, AuxBwdIn{});
}

// GS_FRAME_AUX training frames, every colour model (the rgb row-layout kernel and the SH kernel on the matrix pipe carry no
// depth / alpha terms).  rgb: four waves per SIMD (the depth row and field add ~0.8 KiB of LDS per wave).
// SH: one step fewer than the plain kernel (degree 2: three, degree 3: two waves per SIMD) -- at the plain kernel's budget the
// allocator spilled inside the per-Gaussian loop (tests/test_aux_host.py).
#ifndef GS_BWD_AUX_RGB_WPE
#define GS_BWD_AUX_RGB_WPE 4
#endif
#ifndef GS_BWD_AUX_SH27_WPE
#define GS_BWD_AUX_SH27_WPE 3
#endif
#ifndef GS_BWD_AUX_SH48_WPE
#define GS_BWD_AUX_SH48_WPE 2
#endif
template <int CDIM>
__global__ void __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(CDIM == 48 ? GS_BWD_AUX_SH48_WPE : CDIM == 3 ? GS_BWD_AUX_RGB_WPE : GS_BWD_AUX_SH27_WPE)))
raster_aux_backward_kernel(RasterSrc S, RasterGeom G, BwdIn I, BwdOut O, AuxBwdIn X) {
    raster_backward_pixel_sh_body<CDIM, true, false, true>(S, G, I, O, X);
}

}  // namespace

// One wave per bucket.  Frames: the capped grid, the kernel strides over the work list; reference API: a wave per bucket of
// the list's capacity.  (SH frames take the matrix pipe today: their two instantiations here are built -- their registers
// are pinned by tests/test_kernel_resources.py -- and no frame is sent to them.)
void gs_launch_bwd_pixel(int color_dim, bool frame, int exact, const RasterSrc &S, const RasterGeom &G, const BwdIn &I,
                         const BwdOut &O, int64_t max_buckets, hipStream_t stream) {
    if (frame) {
        gs_for_color_dim(color_dim, [&](auto cd) {
            hipLaunchKernelGGL((raster_backward_pixel_sh_kernel<decltype(cd)::value, true>), dim3(bwd_frame_grid(max_buckets)),
                               dim3(64), 0, stream, S, G, I, O);
        });
        return;
    }
    const dim3 nb((unsigned)(max_buckets > 0 ? max_buckets : 1));
    if (exact && color_dim == 27)
        hipLaunchKernelGGL((raster_backward_pixel_sh_kernel<27, false, true>), nb, dim3(64), 0, stream, S, G, I, O);
    else if (exact)
        hipLaunchKernelGGL((raster_backward_pixel_sh_kernel<3, false, true>), nb, dim3(64), 0, stream, S, G, I, O);
    else if (color_dim == 27)
        hipLaunchKernelGGL((raster_backward_pixel_sh_kernel<27, false>), nb, dim3(64), 0, stream, S, G, I, O);
    else
        hipLaunchKernelGGL((raster_backward_pixel_sh_kernel<3, false>), nb, dim3(64), 0, stream, S, G, I, O);
}

void gs_launch_bwd_aux(int color_dim, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                       const AuxBwdIn &X, int64_t max_buckets, hipStream_t stream) {
    gs_for_color_dim(color_dim, [&](auto cd) {
        hipLaunchKernelGGL(raster_aux_backward_kernel<decltype(cd)::value>, dim3(bwd_frame_grid(max_buckets)), dim3(64), 0,
                           stream, S, G, I, O, X);
    });
}
