// raster_bwd_mfma.hip -- tile rasterizer backward, SH frames: the row layout with the two SH contractions on the matrix pipe,
// its work items, grid and wave policy.  The overview of the backward kernels and the gradient identities: raster_bwd.hip.
#include "raster_bwd_common.h"

namespace {

// SH, frame path: the two contractions of the SH backward on the matrix pipe (raster_backward_mfma_sh_kernel).
//
// Per bucket of 64 Gaussians and tile of 256 pixels the SH backward holds two true matrix products
//   logit[(g, ch)][p]   = sum_k  coef[g][ch][k] sh_k(p)          (64 x 3 rows, K = 9 | 16, 256 columns)
//   dcoef[(g, ch)][k]   = sum_p  D[g][ch][p]   sh_k(p)           (K = 256 pixels: the cross-pixel reduction itself)
// which the pixel-parallel kernel (raster_bwd_pixel.hip) evaluates with 2 x 27 | 48 FMAs per (pixel, Gaussian) on the VALU plus, for the
// second one, a 64 : 1 reduction of 27 | 48 rows through LDS per Gaussian -- together ~3/4 of its ~360 VALU
// instructions per Gaussian step.  An fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered fmaf chain) has the
// VALU's FMA rate but runs BESIDE the VALU and contracts across lanes for free.  The layouts that make both products
// MFMA-shaped at once: a wave works on 16 Gaussians x 16 pixels (one pixel row of the tile) per step,
//   lane l  <->  Gaussian g' = l & 15 of the current group of 16,  pixel quad j = l >> 4  (pixels x = 4 j + i, i = 0..3)
// * colour logits:   D[row = pixel x][col = g'] = sum_k A[x][k] B[k][g'],  A = sh_k(x, y) from an LDS table (lane: x = l & 15,
//   k = 4 kk + (l >> 4)), B = coef[g'][ch][k] (held in registers for the 16 pixel rows).  The result lands exactly where
//   the per-pixel arithmetic wants it: lane (g', j) gets the logits of its four pixels 4 j + reg.
// * coefficient sums: D[row = k][col = g'] += sum_x A'[k][x] B'[x][g'],  B' = D[g'][ch][pixel 4 j + i] -- register i of
//   lane (g', j), as computed --, A' = sh_k(x, y) from the same table (lane: k = l & 15, x = 4 (l >> 4) + i).  The MFMA's
//   K index contracts over the pixel quads, its accumulator over i and over the 16 pixel rows: after 16 steps lane (g', j)
//   holds dL/dcoef[g'][ch][4 j + reg] complete -- no reduction of the coefficient rows through LDS at all.
// What stays on the VALU per (pixel, Gaussian): the Gaussian's value (one v_exp), three sigmoids, the transmittance and
// rho recursions -- over the 16 Gaussians of a group they are a prefix product / prefix sum across the 16 lanes of a DPP
// row (row_shr 1, 2, 4, 8) -- and the seven geometry / opacity sums, which accumulate over the pixel rows in registers
// (dx of a lane's four pixel columns is constant over the rows) and are reduced 4 : 1 once per group.
// A workgroup = one work item (up to GS_MFMA_ITEM_BUCKETS buckets of one tile), W waves; wave w takes buckets w, w + W, ...:
// the SH table (pre-scaled by -log2 e as in the pixel-parallel kernels), dL/dC and the final colours are staged once per item; per
// wave only the pixels' (T, rho) live in LDS
// (read as broadcast float4, written back by the lanes of Gaussian 15 after every pixel row).
// Transmittance: T_before(g') = T_in prod_{h < g'} max(1 - alpha_h, 0) with UNMASKED alphas; a pixel is live while that
// is > 1e-4, exactly the reference's test (gaussian.cu:906) up to the rounding of a product tree against a chain; behind
// the stop every contribution is masked to zero and the unmasked product only ever falls, so it never revives a pixel.
// Waves per workgroup.  A tile of the 376 k-Gaussian scene has two or three buckets, one of the 2.4 M
// scene four or five, a dense one dozens.  Four waves per tile left one or two of their register / LDS slots idle for the
// workgroup's whole life on the short tiles (376 k Gaussians, degree 2: 1.12 ms against 1.00 ms for the pixel-parallel
// kernel); TWO waves: 1.01 ms there, and no worse at 2.4 M Gaussians (1.44 = 1.44 ms at degree 2, 1.46 against 1.50 ms at
// degree 3; the kernel's first version had lost 5 % with two).  Only a small tile grid with long lists wants the four (192
// tiles, 900 pairs each: 0.120 against 0.187 ms): fewer workgroups than the device has slots.  Hence two waves from 1,024
// tiles on, four below.
static inline int gs_bwd_mfma_waves(int n_tiles) { return n_tiles >= 1024 ? 2 : 4; }
#ifndef GS_BWD_MFMA_WPE
#define GS_BWD_MFMA_WPE 3
#endif

// (the DPP row scans of the row-layout kernels, gs_row_scan_add4_oop / gs_row_scan_mul4_excl: raster_common.h)
// workgroups of the matrix-pipe launch: one per work item up to 2 T (the kernel walks the items with the grid as the stride;
// the executed-row counters have GS_BWD_EXEC_SLOTS x T = 8 T slots for grid x waves)
static_assert(4 <= GS_BWD_EXEC_SLOTS, "executed-row counters");
static inline unsigned gs_bwd_mfma_grid(int n_tiles, int64_t max_buckets) {
    const int64_t cap_items = n_tiles + max_buckets / GS_MFMA_ITEM_BUCKETS;
    return (unsigned)(cap_items < 2ll * n_tiles ? cap_items : 2ll * n_tiles);
}
// The row step (round 5's instruction diet, first used by raster_backward_rows_kernel, raster_bwd_rows.hip): the opacity in the exponent's
// constant term (no G x opacity product), T in front of the Gaussian as one DPP multiply, s = w gc - rho beta; the per-pixel
// algebra between the two matrix products runs on PAIRS of the lane's four pixels (packed fp32); the scans, the
// transcendentals and the stop-point selects stay per pixel.
template <int CDIM, int W>
__global__ void __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(GS_BWD_MFMA_WPE)))
raster_backward_mfma_sh_kernel(RasterSrc S, RasterGeom G, BwdIn I, BwdOut O) {
    static_assert(CDIM == 27 || CDIM == 48, "SH colours only");
    // tiles per workgroup, and workgroups per tile.  Both were experiments (two tiles sharing one workgroup's waves; two
    // workgroups per tile: 1.61 / 1.67 against 1.44 / 1.46 ms) and are 1 for good; the loops below still run over them
    // because writing them out flat changed the register allocation of all four instantiations (tools/isa_diff.py)
    constexpr int TPW = 1;
    constexpr int NB = CDIM / 3;          // basis functions per channel: 9 | 16
    constexpr int KQ = NB / 4;            // k blocks of four of the colour product on the matrix pipe: 2 | 4
    // degree 2 has nine basis functions: the ninth would cost a third, three-quarters empty MFMA per channel (14 ns each);
    // it enters the logits as the MFMAs' initial accumulator instead, sh'_8(pixel) coef[ch][8]: 12 multiplications
    constexpr bool TAIL = NB % 4 != 0;
    static_assert(!TAIL || NB == 4 * KQ + 1, "one basis function beside the blocks of four");
    constexpr int P = 17;                 // floats per pixel in the SH table (16 + 1: both operand patterns nearly conflict-free)
    constexpr int RW = gs_row_floats(CDIM);
    constexpr uint32_t GS_NO_SLOT = 0xffffffffu;
    typedef float f4 __attribute__((ext_vector_type(4)));
    __shared__ float s_sh[TPW][256 * P];                                 // [pixel 16 y + x][k], entries k >= NB are zero
    __shared__ __attribute__((aligned(16))) float s_gr[TPW][3][256];    // dL/dC (masked: crop, clamp)
    __shared__ float s_py[TPW][16];
    __shared__ __attribute__((aligned(16))) float s_sh8[TAIL ? TPW : 1][TAIL ? 256 : 4];  // sh'_(NB - 1) of the pixel
    __shared__ __attribute__((aligned(16))) float s_T[W][256];          // per wave: transmittance / rho in front of the current group
    __shared__ __attribute__((aligned(16))) float s_rho[W][256];
    auto lds_order = [] {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Work items (round 5): (tile, first bucket, buckets) with at most GS_MFMA_ITEM_BUCKETS buckets, in the forward's dispatch
    // order of the tiles (heavy tiles first), built by mfma_items_kernel underneath the caller's loss.  One workgroup per TILE
    // (round 4) walks a tile's buckets W at a time, so the kernel lasts as long as its longest tile: on the 2.4 M scene
    // (3.8 buckets per tile on average, 14 at most) that is harmless, in a densifying run it is not -- a few tiles with 30 - 100
    // buckets kept one workgroup busy for milliseconds while the device idled (kernel trace of tools/soak.py, SH degree 2:
    // 1.78 ms per call on average, 5.4 ms at worst, at 376 k - 556 k Gaussians; 1.27 ms at 2.4 M Gaussians, profiles/r05_j_*).
    // A workgroup takes items blockIdx.x, + gridDim.x, ... and rebuilds the tile's tables per item (a few microseconds
    // against >= 56 us per bucket).  Without an item list (I.mfma_items = NULL): one item per tile, as before.
    const uint32_t n_tiles = (uint32_t)(G.ntx * G.nty);
    constexpr uint32_t SPLIT = 1;
    const uint32_t n_items = I.mfma_items ? *I.mfma_n_items : gridDim.x;
    uint32_t n_exec = 0;  // (wave-uniform) pixel-row steps this wave executed: what its MFMA flops are counted from
    constexpr float KS = -GS_LOG2E;  // the table holds sh'_k = -log2(e) sh_k (raster_common.h)
    const uint32_t gq = (uint32_t)lane & 15u, jq = (uint32_t)lane >> 4;  // Gaussian of the group, pixel quad
    float *sT = s_T[wave], *sR = s_rho[wave];
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    uint32_t tile0, bk0 = 0, part = 0;
    // the workgroup's TPW consecutive tiles: their buckets form ONE work list that the W waves share (a tile has 4.3
    // buckets on average at 2.4 M Gaussians: alone it keeps four waves busy 68 % of the time, two tiles together 85 %)
    uint32_t nbk[TPW], nproc_t[TPW], total_bk = 0;
    if (TPW == 1 && I.mfma_items) {
        const uint4 it = I.mfma_items[item];
        tile0 = it.x;
        bk0 = it.y;
        nproc_t[0] = I.tile_nproc[tile0];
        nbk[0] = total_bk = it.z;
    } else {
        const uint32_t wg = item / SPLIT;
        part = item % SPLIT;  // workgroup `part` of SPLIT of this tile
        tile0 = (TPW == 1 && I.tile_order) ? I.tile_order[wg] : wg * TPW;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            nproc_t[t] = tile0 + t < n_tiles ? I.tile_nproc[tile0 + t] : 0;
            nbk[t] = (nproc_t[t] + GS_BUCKET - 1) / GS_BUCKET;
            total_bk += nbk[t];
        }
    }
    if (total_bk <= part * W) continue;  // uniform: nothing (left) of these tiles for this workgroup
    __syncthreads();  // (a wave of this workgroup may still be reading the previous item's tables)

    // ---- per tile: SH table, dL/dC, pixel-row centres
    for (int q = tid; q < 256 * TPW; q += 64 * W) {
        const int t = q >> 8, p = q & 255;
        if (nbk[t] == 0) continue;
        const uint32_t tile = tile0 + t, tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
        const uint32_t id_x = tx * 16 + (p & 15), id_y = ty * 16 + (p >> 4);
        float sh[NB];
        raster_pixel_sh<NB>(id_x, id_y, G, sh);
#pragma unroll
        for (int k = 0; k < 16; ++k) s_sh[t][p * P + k] = k < NB ? KS * sh[k < NB ? k : 0] : 0.f;
        if (TAIL) s_sh8[t][p] = KS * sh[NB - 1];
        float f[3], gr[3];
        load_pixel_inputs<true>(I, G, id_x, id_y, f, gr);
#pragma unroll
        for (int e = 0; e < 3; ++e) s_gr[t][e][p] = gr[e];
    }
    if (tid < 16 * TPW) {
        const uint32_t tile = tile0 + (tid >> 4);
        s_py[tid >> 4][tid & 15] = raster_pixel_coord((tile / (uint32_t)G.ntx) * 16 + (tid & 15), G.padH, G.focal_y);
    }
    __syncthreads();

    for (uint32_t u = part * W + wave; u < total_bk; u += W * SPLIT) {
        int t = 0;
        uint32_t b = bk0 + u;
#pragma unroll
        for (int k = 0; k + 1 < TPW; ++k)
            if (t == k && b >= nbk[k]) {
                b -= nbk[k];
                t = k + 1;
            }
        const uint32_t tile = tile0 + t, nproc = nproc_t[t];
        const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
        const uint32_t start = (uint32_t)I.ranges[2 * tile];
        const float *tab = s_sh[t], *gr0 = s_gr[t][0], *gr1 = s_gr[t][1], *gr2 = s_gr[t][2], *pyt = s_py[t];
        const float *tab8 = s_sh8[TAIL ? t : 0];
        const uint32_t base = b * GS_BUCKET, rem = nproc - base, r = rem < GS_BUCKET ? rem : GS_BUCKET;
        // the bucket's 64 Gaussian ids, one per lane: a group learns its ids from a lane exchange instead of a load that
        // everything else of the group's set-up would wait for
        const uint32_t id_lane = S.ids[start + base + ((uint32_t)lane < r ? (uint32_t)lane : r - 1)];
        // ---- pixel states at the bucket's boundary: the forward's checkpoint ((1, 0) in front of the tile's first bucket)
        {
            const float4 *ck = I.ckpt + raster_ckpt_slot(start, tile, b) * 256;
            float4 c[4];
            float f[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[k] = b == 0 ? make_float4(1.f, 0.f, 0.f, 0.f) : ck[64 * k + lane];
                // pixel (x = lane & 15, y = (lane >> 4) + 4 k) == index 64 k + lane of the tile
                const float *cf = I.c_final + ((size_t)(ty * 16 + (lane >> 4) + 4 * k) * G.padW + tx * 16 + (lane & 15)) * 3;
                f[k][0] = cf[0];
                f[k][1] = cf[1];
                f[k][2] = cf[2];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = 64 * k + lane;
                sT[p] = c[k].x;
                sR[p] = gr0[p] * (f[k][0] - c[k].y) + gr1[p] * (f[k][1] - c[k].z) + gr2[p] * (f[k][2] - c[k].w);
            }
        }
        lds_order();
        const uint32_t ngrp = (r + 15) / 16;
        for (uint32_t grp = 0; grp < ngrp; ++grp) {
            // ---- this lane's Gaussian (entries beyond r re-read the bucket's last one with opacity 0: alpha = 0)
            const uint32_t gi = grp * 16 + gq;
            const bool valid = gi < r;
            const uint32_t gid = (uint32_t)__shfl((int)id_lane, (int)(valid ? gi : r - 1), 64);
            GaussianRec g;
            {
                const float4 ge = S.geom[(size_t)gid * GS_REC_STRIDE], cv = S.cov4[(size_t)gid * GS_REC_STRIDE];
                g.x = ge.x;
                g.y = ge.y;
                g.opa = ge.w;
                g.a = cv.x;
                g.b = cv.y;
                g.c = cv.z;
                g.d = cv.w;
            }
            const float *cf = S.sh + (size_t)gid * CDIM;
            float cob[3][KQ];  // B operand of the colour product: coef[g'][ch][4 kk + jq]
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int kk = 0; kk < KQ; ++kk) {
                    const uint32_t k = 4 * kk + jq;
                    cob[ch][kk] = (4 * kk + 3 < NB || k < (uint32_t)NB) ? cf[ch * NB + (k < (uint32_t)NB ? k : 0)] : 0.f;
                }
            float ctail[3] = {0.f, 0.f, 0.f};
            if (TAIL) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) ctail[ch] = cf[ch * NB + NB - 1];
            }
            // the next group's coefficient rows (192 bytes = three lines per Gaussian at degree 3; 2.4 M of them do not
            // fit the Infinity Cache) and records are asked for now, one line per lane, and nothing waits for them: by the
            // time the next group sets up they sit in L2
            float warm = 0.f;
            if (grp + 1 < ngrp) {
                const uint32_t gn = (grp + 1) * 16 + gq;
                const uint32_t idn = (uint32_t)__shfl((int)id_lane, (int)(gn < r ? gn : r - 1), 64);
                warm = jq * 16 < (uint32_t)CDIM ? S.sh[(size_t)idn * CDIM + jq * 16]
                                                : reinterpret_cast<const float *>(S.geom + (size_t)idn * GS_REC_STRIDE)[0];
            }
            float cA, cB, cC;
            raster_conic(g, cA, cB, cC);
            const float lopa = fmaxf(__log2f(g.opa), -200.0f);
            uint32_t slot = GS_NO_SLOT;
            if (valid) {
                const uint4 rc = O.rects[gid];
                const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16;
                const uint64_t sl = (uint64_t)O.pair_offsets[gid] + (ty - y0) * (x1 - x0) + (tx - x0);
                if (sl < O.max_pairs) slot = (uint32_t)sl;
            }
            // (what only the group's closing needs -- dx, the covariance, two of the conic's terms -- is recomputed /
            // re-read there instead of living in registers through the 16 pixel rows: the loop sits at the register
            // limit of three waves per SIMD)
            float bdx[4], adx2[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dxi = raster_pixel_coord(tx * 16 + 4 * jq + i, G.padW, G.focal_x) - g.x;
                bdx[i] = cB * dxi;
                adx2[i] = cA * dxi * dxi;
                // q' = q - log2 sigma(opa): alpha = 2^-q'.  A padded entry: q' = 1e30 => alpha = 0 exactly, 0 x 1e30 = 0 in
                // the sum of s q'; an opacity that underflowed to 0: 2^-(q + 200) is flushed to 0
                adx2[i] = valid ? adx2[i] - lopa : 1e30f;
            }
            const float gy = g.y;
            f4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            float S1[4] = {0.f, 0.f, 0.f, 0.f}, Sy[4] = {0.f, 0.f, 0.f, 0.f}, Syy = 0.f, Sq = 0.f;  // (S1, Sy, Sq: unpacked behind the loop)
            typedef float f2 __attribute__((ext_vector_type(2)));
            auto pfma = [](f2 x, f2 y, f2 z) { return __builtin_elementwise_fma(x, y, z); };
            f2 S1p[2] = {{0.f, 0.f}, {0.f, 0.f}}, Syp[2] = {{0.f, 0.f}, {0.f, 0.f}}, Sqp = {0.f, 0.f};
            // The LDS operands of a pixel row -- the A operands of both products, the row's pixel states and dL/dC -- are
            // requested one row ahead, behind the row's arithmetic and in front of its twelve coefficient MFMAs (registers
            // are free there, and the ~100 cycles of LDS latency pass under the MFMAs; asked for where they are used,
            // every row started and ended with an exposed wait).
            float a_n[KQ], tb_n[4];
            f4 Tin_n, Rin_n, G0_n, G1_n, G2_n, S8_n = {0.f, 0.f, 0.f, 0.f};
            auto row_loads = [&](int s) {
                const int prow = 16 * s;
#pragma unroll
                for (int kk = 0; kk < KQ; ++kk) a_n[kk] = tab[(prow + (int)gq) * P + 4 * kk + (int)jq];  // l & 15: pixel column
#pragma unroll
                for (int i = 0; i < 4; ++i) tb_n[i] = tab[(prow + 4 * (int)jq + i) * P + (int)gq];       // l & 15: basis function
                Tin_n = *reinterpret_cast<const f4 *>(sT + prow + 4 * jq);
                Rin_n = *reinterpret_cast<const f4 *>(sR + prow + 4 * jq);
                G0_n = *reinterpret_cast<const f4 *>(gr0 + prow + 4 * jq);
                G1_n = *reinterpret_cast<const f4 *>(gr1 + prow + 4 * jq);
                G2_n = *reinterpret_cast<const f4 *>(gr2 + prow + 4 * jq);
                if (TAIL) S8_n = *reinterpret_cast<const f4 *>(tab8 + prow + 4 * jq);
            };
            row_loads(0);
            for (int s = 0; s < 16; ++s) {  // pixel row s of the tile
                const int prow = 16 * s;
                float a[KQ], tb[4];
#pragma unroll
                for (int kk = 0; kk < KQ; ++kk) a[kk] = a_n[kk];
#pragma unroll
                for (int i = 0; i < 4; ++i) tb[i] = tb_n[i];
                const f4 Tin = Tin_n, Rin = Rin_n, G0 = G0_n, G1 = G1_n, G2 = G2_n, S8 = S8_n;
                // A pixel row whose 16 pixels have all stopped (T <= 1e-4 in front of the group: the transmittance only
                // falls) adds exact zeros to every sum of every Gaussian of the group and its states need not move: the
                // row is left out (wave-uniform).  The tile's list ends where its LAST pixel stops, so at 2.4 M Gaussians a
                // good part of the rows of a tile's later groups are of this kind.
                if (__ballot(Tin[0] > GS_T_STOP || Tin[1] > GS_T_STOP || Tin[2] > GS_T_STOP || Tin[3] > GS_T_STOP) == 0ull) {
                    if (s + 1 < 16) row_loads(s + 1);
                    continue;
                }
                ++n_exec;
                // colour logits of (pixel 4 jq + reg, Gaussian gq) on the matrix pipe
                f4 lg[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                if (TAIL) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) lg[ch] = S8 * ctail[ch];
                }
#pragma unroll
                for (int kk = 0; kk < KQ; ++kk)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) lg[ch] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], cob[ch][kk], lg[ch], 0, 0, 0);
                const float dy = pyt[s] - gy;
                const f2 dy2 = {dy, dy};
                f4 Tout, Rout;
                float dv[3][4];
                f2 q2[2];
                float araw[4], pin[4], Tb[4];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    q2[h] = pfma(pfma(f2{cC, cC}, dy2, -f2{bdx[2 * h], bdx[2 * h + 1]}), dy2, f2{adx2[2 * h], adx2[2 * h + 1]});
                    araw[2 * h] = gs_exp2(-q2[h].x);  // (q is q' = q - log2 sigma(opa): 2^-q' is alpha itself)
                    araw[2 * h + 1] = gs_exp2(-q2[h].y);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // (0 <= 1 - alpha <= 1 holds anyway for sane records; written as a clamp to [0, 1] it is the clamp
                    // modifier of the subtraction, one instruction -- and a NaN / > 1 alpha of a broken record stops the pixel)
                    pin[i] = fminf(fmaxf(1.0f - araw[i], 0.f), 1.0f);
                    Tb[i] = Tin[i];
                }
                // transmittance in front of this Gaussian: T_in times the product over the group's earlier Gaussians
                gs_row_scan_mul4_excl(pin, Tb);
                float alpha[4], wg[4], wsum[4];
                f2 w2[2], al2[2], cc2[3][2];
#pragma unroll
                for (int i = 0; i < 4; ++i) alpha[i] = Tb[i] > GS_T_STOP ? araw[i] : 0.f;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    al2[h] = f2{alpha[2 * h], alpha[2 * h + 1]};
                    w2[h] = al2[h] * f2{Tb[2 * h], Tb[2 * h + 1]};
                    // colours sigma(logit) = 1 / (1 + 2^(logit')) with the pre-scaled basis
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const f2 den = f2{1.0f, 1.0f} + f2{gs_exp2(lg[ch][2 * h]), gs_exp2(lg[ch][2 * h + 1])};
                        cc2[ch][h] = f2{gs_rcp(den.x), gs_rcp(den.y)};
                    }
                    const f2 g0 = h ? G0.zw : G0.xy, g1 = h ? G1.zw : G1.xy, g2 = h ? G2.zw : G2.xy;
                    const f2 wgh = w2[h] * pfma(g2, cc2[2][h], pfma(g1, cc2[1][h], g0 * cc2[0][h]));
                    wg[2 * h] = wgh.x;
                    wg[2 * h + 1] = wgh.y;
                    const f2 to = (h ? Tin.zw : Tin.xy) * f2{pin[2 * h], pin[2 * h + 1]};  // (lanes of Gaussian 15: the group's product)
                    Tout[2 * h] = to.x;
                    Tout[2 * h + 1] = to.y;
                }
                gs_row_scan_add4_oop(wsum, wg);  // rho behind this Gaussian: rho_in minus the inclusive prefix sum of w gc
                f2 svs[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f2 rho = (h ? Rin.zw : Rin.xy) - f2{wsum[2 * h], wsum[2 * h + 1]};
                    const f2 den = f2{1.00000011920928955f, 1.00000011920928955f} - f2{araw[2 * h], araw[2 * h + 1]};
                    // s = dL/dalpha alpha = w gc - rho beta, beta = alpha / (1 - alpha + 1e-7): masked with alpha, like w
                    const f2 sv = pfma(-rho, al2[h] * f2{gs_rcp(den.x), gs_rcp(den.y)}, f2{wg[2 * h], wg[2 * h + 1]});
                    // (the opacity sum, sum of dL/dalpha G over the live pixels, is sum of s / opacity: at the group's end)
                    // D = dL/dC_ch w c (1 - c) [x -ln 2: D sh' = D' sh]
                    const f2 wk = w2[h] * f2{-GS_LN2, -GS_LN2};
                    const f2 g0 = h ? G0.zw : G0.xy, g1 = h ? G1.zw : G1.xy, g2 = h ? G2.zw : G2.xy;
                    const f2 d0 = (g0 * wk) * pfma(-cc2[0][h], cc2[0][h], cc2[0][h]);
                    const f2 d1 = (g1 * wk) * pfma(-cc2[1][h], cc2[1][h], cc2[1][h]);
                    const f2 d2 = (g2 * wk) * pfma(-cc2[2][h], cc2[2][h], cc2[2][h]);
                    dv[0][2 * h] = d0.x, dv[0][2 * h + 1] = d0.y;
                    dv[1][2 * h] = d1.x, dv[1][2 * h + 1] = d1.y;
                    dv[2][2 * h] = d2.x, dv[2][2 * h + 1] = d2.y;
                    S1p[h] += sv;
                    Syp[h] = pfma(sv, dy2, Syp[h]);
                    Sqp = pfma(sv, q2[h], Sqp);
                    svs[h] = sv;
                    Rout[2 * h] = rho.x;
                    Rout[2 * h + 1] = rho.y;
                }
                const f2 ss = svs[0] + svs[1];
                Syy = fmaf((ss.x + ss.y) * dy, dy, Syy);
                if (s + 1 < 16) {
                    row_loads(s + 1);
                    __builtin_amdgcn_sched_barrier(0);  // (the requests stay in front of the MFMAs below)
                }
                // coefficient sums: acc[ch][reg] += sum over the row's 16 pixels of D[ch] sh'_(4 jq + reg)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = __builtin_amdgcn_mfma_f32_16x16x4f32(tb[i], dv[ch][i], acc[ch], 0, 0, 0);
                if (gq == 15) {  // the row's pixel states in front of the next group
                    *reinterpret_cast<f4 *>(sT + prow + 4 * jq) = Tout;
                    *reinterpret_cast<f4 *>(sR + prow + 4 * jq) = Rout;
                }
            }
            asm volatile("" ::"v"(warm));  // (the warming load must not be dropped; its value is not used)
            S1[0] = S1p[0].x, S1[1] = S1p[0].y, S1[2] = S1p[1].x, S1[3] = S1p[1].y;
            Sy[0] = Syp[0].x, Sy[1] = Syp[0].y, Sy[2] = Syp[1].x, Sy[3] = Syp[1].y;
            Sq = Sqp.x + Sqp.y;
            // ---- close the group: the lane's four pixel columns, then the four pixel quads of the Gaussian
            const uint32_t gid2 = (uint32_t)__shfl((int)id_lane, (int)(valid ? gi : r - 1), 64);
            const float4 ge2 = S.geom[(size_t)gid2 * GS_REC_STRIDE], cv2 = S.cov4[(size_t)gid2 * GS_REC_STRIDE];
            float Sx = 0.f, Sxx = 0.f, Sxy = 0.f, Syt = 0.f;
            // s = dL/dalpha alpha and alpha = G sigma(opa) on every live pixel: sum dL/dalpha G = (sum s) / sigma(opa).  (An
            // opacity that underflowed to 0 composites nothing; its derivative sigma (1 - sigma) downstream is 0 as well.)
            float Sopa = ((S1[0] + S1[1]) + (S1[2] + S1[3])) * (ge2.w > 0.f ? gs_rcp(ge2.w) : 0.f);
            const float lopa2 = fmaxf(__log2f(ge2.w), -200.0f);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dxi = raster_pixel_coord(tx * 16 + 4 * jq + i, G.padW, G.focal_x) - ge2.x;
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
            Sopa = quad_sum(Sopa);
            // ---- the group's 16 rows leave as whole 64-byte lines (round 5; row layout: gs_frame_layout.h).  A row is spread
            // over the four lanes (g, jq) of its Gaussian; line `it` of the row is put together from one 16-byte piece of each
            // of them -- destination lane 4 r + q takes the piece of lane (g = r, jq = q) through four ds_bpermute -- and
            // stored by ONE instruction, four lanes x 16 bytes per line, sixteen rows per instruction: every line reaches
            // the memory system complete (round 4: twelve scalar stores per lane at a 28-byte offset into rows that straddle
            // lines and a flag byte per row -- PMC WRITE_SIZE 2.2 x / 1.32 x the row bytes).  The geometry algebra runs in
            // all four lanes of a Gaussian (they hold the same sums after quad_sum): whichever lane carries a header piece
            // has it.
            float h0[4], h1[4];  // header pieces (dx, dy, da, db), (dc, dd, dopa, 0)
            {
                const float a = cv2.x, bb = cv2.y, cc = cv2.z, d = cv2.w;
                float cA, cB, cC;
                gs_conic(a, bb, cc, d, cA, cB, cC);
                const float iPn = 1.0f / (2.0f * raster_det(a, bb, cc, d) + 1e-14f);
                // (the loop summed s q' with q' = q - log2 sigma(opa); Sopa x sigma(opa) is the sum of s)
                const float Su = fmaf(lopa2, Sopa * ge2.w, Sq) * GS_LN2;
                h0[0] = GS_LN2 * (2.0f * cA * Sx - cB * Syt);
                h0[1] = GS_LN2 * (2.0f * cC * Syt - cB * Sx);
                h0[2] = iPn * (-Syy + 2.0f * d * Su);
                h0[3] = iPn * (Sxy - 2.0f * cc * Su);
                h1[0] = iPn * (Sxy - 2.0f * bb * Su);
                h1[1] = iPn * (-Sxx + 2.0f * a * Su);
                h1[2] = Sopa;
                h1[3] = 0.f;
            }
            {
                const int dr = lane >> 2, dq = lane & 3, src = dr + 16 * dq;  // destination row / piece, its source lane
                const uint32_t dslot = (uint32_t)__shfl((int)slot, dr, 64);
                float4 *drow = reinterpret_cast<float4 *>(O.rows + (size_t)(dslot != GS_NO_SLOT ? dslot : 0) * RW);
                auto put = [&](int line, const float v[4]) {  // this lane OFFERS v; lane 4 r + q stores what lane (r, q) offers
                    float4 o;
                    o.x = __shfl(v[0], src, 64);
                    o.y = __shfl(v[1], src, 64);
                    o.z = __shfl(v[2], src, 64);
                    o.w = __shfl(v[3], src, 64);
                    if (dslot != GS_NO_SLOT) drow[4 * line + dq] = o;
                };
                if constexpr (NB == 16) {
                    // line 0: the header, pieces 0 / 1 from lanes jq = 0 / 1, zeros from the others; line 1 + ch: coef(ch, 0..15)
                    float hv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) hv[e] = jq == 0 ? h0[e] : jq == 1 ? h1[e] : 0.f;
                    put(0, hv);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float cv[4] = {acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
                        put(1 + ch, cv);
                    }
                } else {
                    // line ch: coef(ch, 0..11) from lanes jq = 0..2 (k >= 9: the table's zero entries: exact zeros), header
                    // piece ch from lane jq = 3, which has no coefficient
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float cv[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) cv[e] = jq == 3 ? (ch == 0 ? h0[e] : ch == 1 ? h1[e] : 0.f) : acc[ch][e];
                        put(ch, cv);
                    }
                }
            }
        }
        lds_order();  // (the next bucket's states overwrite this wave's arrays)
    }
    }  // work items
    if (lane == 0) O.exec_rows[(size_t)blockIdx.x * W + wave] = n_exec;
}

// The SH backward's work items: (tile, first bucket, buckets <= chunk) in the forward's dispatch order of the tiles (`order`:
// heavy tiles first; NULL: raster order).  A long list becomes several items, i.e. several workgroups.
__global__ void __launch_bounds__(1024) mfma_items_kernel(const uint32_t *__restrict__ tile_nproc, int n_tiles,
                                                         const uint32_t *__restrict__ order, uint32_t chunk,
                                                         uint4 *__restrict__ items, uint32_t *__restrict__ n_items) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < n_tiles; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t tile = i < n_tiles ? (order ? order[i] : (uint32_t)i) : 0u;
        const uint32_t nb = i < n_tiles ? (tile_nproc[tile] + GS_BUCKET - 1) / GS_BUCKET : 0u;
        const uint32_t v = (nb + chunk - 1) / chunk;
        const uint32_t incl = gs_wave_incl_scan_u32(v);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t woff = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) woff += w < wave ? s_wave[w] : 0;
        const uint32_t carry = s_carry, first = carry + woff + incl - v;
        for (uint32_t c = 0; c < v; ++c) {
            const uint32_t b0 = c * chunk, left = nb - b0;
            items[first + c] = make_uint4(tile, b0, left < chunk ? left : chunk, 0u);
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_items = s_carry;
}

}  // namespace

// one workgroup per work item (a long list is several items, spread over the device: nothing is handed to another kernel)
void gs_launch_bwd_mfma(int color_dim, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                        int64_t max_buckets, hipStream_t stream) {
    const int n_tiles = G.ntx * G.nty;
    const dim3 grid(gs_bwd_mfma_grid(n_tiles, max_buckets));
    auto launch = [&](auto cd) {
        constexpr int CD = decltype(cd)::value;
        if (gs_bwd_mfma_waves(n_tiles) == 2)
            hipLaunchKernelGGL((raster_backward_mfma_sh_kernel<CD, 2>), grid, dim3(128), 0, stream, S, G, I, O);
        else
            hipLaunchKernelGGL((raster_backward_mfma_sh_kernel<CD, 4>), grid, dim3(256), 0, stream, S, G, I, O);
    };
    if (color_dim == 48)
        launch(gs_int<48>{});
    else
        launch(gs_int<27>{});
}

void gs_launch_mfma_items(const uint32_t *tile_nproc, int n_tiles, const uint32_t *order, uint4 *items, uint32_t *n_items,
                          hipStream_t stream) {
    hipLaunchKernelGGL(mfma_items_kernel, dim3(1), dim3(1024), 0, stream, tile_nproc, n_tiles, order,
                       (uint32_t)GS_MFMA_ITEM_BUCKETS, items, n_items);
}

// (workgroup, wave) slots the SH backward on the matrix pipe writes its executed-row counters to (0: this colour model
// takes another kernel): the launch geometry of gs_launch_bwd_mfma
int gs_bwd_mfma_slots(int color_dim, int n_tiles, int64_t max_buckets) {
    if (color_dim != 27 && color_dim != 48) return 0;
    return (int)gs_bwd_mfma_grid(n_tiles, max_buckets) * gs_bwd_mfma_waves(n_tiles);
}
