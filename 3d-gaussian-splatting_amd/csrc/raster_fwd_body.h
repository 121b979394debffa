// raster_fwd_body.h -- 16x16-tile front-to-back alpha compositing, forward: the kernel.
//
// raster_forward_body, its two __global__ wrappers (raster_forward_kernel, raster_aux_forward_kernel) and launch_fwd.
// Included by the two files that launch them, each of which instantiates only what it launches: raster_fwd.hip (the frame
// path, FRAME = true) and raster_fwd_ref.hip (the reference API, FRAME = false).
//
// Replaces draw_kernel (gaussian.cu:806-970).  One wave64 per tile, four pixels per lane.  The tile's sorted
// Gaussian list is streamed through LDS in chunks with a two-deep ring: every thread gathers
// one Gaussian of the NEXT chunk from HBM/L2 into registers while the waves composite the
// current chunk out of LDS (broadcast ds_read_b128), so a chunk costs a single barrier.
// Differences from the reference kernel, all numerically neutral at fp32 tolerance:
//   * the per-pixel fp64 division by (2 det + 1e-14) is hoisted to once per (tile, Gaussian)
//     and the exponent is pre-scaled by log2(e) so the pixel loop issues one v_exp_f32;
//   * early termination is wave-uniform (ballot) with exact per-pixel masking, and the
//     inter-chunk shared-memory race of the reference (no barrier after its compute loop,
//     gaussian.cu:878-962) cannot occur: the ring buffer is only rewritten one barrier later;
//   * in training mode the kernel also stores the per-pixel state (T, C) at every 64-Gaussian
//     bucket boundary; the backward pass uses these checkpoints to process buckets
//     independently (raster_bwd.hip).
#pragma once
#include <type_traits>

#include "raster_fwd_common.h"

namespace {

// Lane l owns the four pixels (x, y0 + 4k), k = 0..3, of the tile, x = l & 15, y0 = l >> 4; pixel
// index inside the tile p_k = 64 k + l.  The compositing loop is bound by fp32 VALU ISSUE (PMC: ~31 VALU
// wave-instructions per Gaussian step of 256 pixels, 28 of them arithmetic; the same instruction stream fed from
// registers without any memory access runs at the same speed, tools/ubench/raster_feed.hip), so the layout is chosen
// to share work between pixels: dx and the three dx-only terms of the exponent are computed once per lane for four
// pixels, the per-Gaussian operands are read from LDS once per lane (broadcast ds_read_b128, four Gaussians per
// read) and the fp32 math is packed over pixel PAIRS (v_pk_*_f32).  With a single wave per tile there is no workgroup
// barrier at all; the staging of the next chunk (one Gaussian per lane) overlaps the compositing of the current one
// through registers.
// The kernel is PERSISTENT: the grid is a few waves per SIMD and every wave walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  While a wave composites the LAST chunk of its tile it already gathers
// chunk 0 of its NEXT tile, so the dependent id -> record gather latency (and the per-tile range load)
// sits behind math instead of in front of it.  With one tile per wave all waves run their gather,
// math and store phases in lockstep and the phases add up instead of overlapping.
//
// The body of the compositing kernel.  AUX = true (raster_aux_forward_kernel): two more accumulators per pixel -- D = sum w d
// with d = rec_geom.z staged in LDS as one more field, and A = sum w accumulated exactly like a colour channel of value
// 1.0 -- with their checkpoints and maps; everything else (stop, cut table, order, statistics) as in the plain kernel.
// AUX = false compiles to the plain kernel unchanged.
template <int CDIM, bool FRAME, bool CKPT, bool SIG, bool WN, bool EXACT, bool AUX, bool COMPACT = false>
__device__ __forceinline__ void raster_forward_body(RasterSrc S, RasterGeom G,
                                                    const int32_t *__restrict__ ranges,
                                                    float *__restrict__ out_padded,
                                                    float *__restrict__ out_image,
                                                    float4 *__restrict__ ckpt,
                                                    uint32_t *__restrict__ tile_nproc,
                                                    uint32_t n_tiles,
                                                    float4 *__restrict__ cont_state,
                                                    uint32_t *__restrict__ cont_flag,
                                                    const uint32_t *__restrict__ tile_order,
                                                    uint32_t *__restrict__ tile_cost,
                                                    const uint32_t *cut_in, uint32_t *cut_out,
                                                    unsigned long long *__restrict__ ranpast,
                                                    const unsigned long long *__restrict__ gate,
                                                    const AuxFwdOut &X, uint32_t compact_min = 0,
                                                    uint32_t *__restrict__ tile_compact = nullptr) {
    static_assert(!COMPACT || (CDIM == 3 && FRAME && !CKPT && !SIG && !WN && !EXACT && !AUX),
                  "the compact phase belongs to the rgb inference frame");
    static_assert(!AUX || (FRAME && !SIG && !WN && !EXACT), "depth / alpha maps belong to the frame path");
    static_assert(!(EXACT && FRAME), "the exact-exp flavour belongs to the reference API (gs_draw, fast = 0)");
    // frame path, temporal occlusion cull (gs_frame_layout.h): `cut_out` [T] receives, per tile, the depth behind which this
    // launch composited nothing (all its pixels had stopped) or GS_NO_CUT; `cut_in` (the same table, set when this frame's
    // lists were trimmed by it) makes a tile that reaches the end of its list with a live pixel, or that composited a Gaussian
    // behind its cut, raise *ranpast; `gate`: the untrimmed second pass, which only runs if some tile did
    if (FRAME && gate && *gate == 0) return;
    using SM = FwdSmem<CDIM>;
    constexpr int CH = SM::CH;
#ifndef GS_FWD_GROUP
#define GS_FWD_GROUP 4
#endif
    // Gaussians per LDS read of a field (ds_read_b128: 4, ds_read_b64: 2 -- half the operand registers; A/B switch)
    constexpr uint32_t GROUP = CDIM == 3 ? GS_FWD_GROUP : 4;
    static_assert(GROUP == 4 || GROUP == 2, "GROUP");
    // the wave-uniform liveness test (3 VALU instructions + a branch) runs before every second group without SH;
    // with SH a Gaussian step is an order of magnitude longer and every group is tested
#ifndef GS_FWD_LIVE_EVERY
#define GS_FWD_LIVE_EVERY 8
#endif
    constexpr uint32_t LIVE_EVERY = CDIM == 3 ? GS_FWD_LIVE_EVERY : 4;
    __shared__ SM sm;
    __shared__ float s_dep[AUX ? SM::NBUF : 1][AUX ? CH : 1] __attribute__((aligned(16)));  // AUX: d of the chunk's Gaussians
    // COMPACT: the hand-over area of the compact phase (below), one entry per live pixel: T, three colour sums, the pixel's x
    // and y coordinate and its index in the tile; 3.5 KiB beside FwdSmem<3>: 16 one-wave workgroups per CU still fit
    enum { KT, KR, KG, KB, KX, KY, KI, KFIELD };
    constexpr int KCAP = 128;
    __shared__ float s_cmp[COMPACT ? KFIELD : 1][COMPACT ? KCAP : 1] __attribute__((aligned(16)));
    const int lane = threadIdx.x;

    auto range_of = [&](uint32_t t, uint32_t &s0, uint32_t &cnt) {
        s0 = cnt = 0;
        if (t < n_tiles) {
            s0 = (uint32_t)(FRAME ? ranges[2 * t] : ranges[t]);
            cnt = (uint32_t)(FRAME ? ranges[2 * t + 1] : ranges[t + 1]) - s0;
        }
    };
    // Dispatch order (frame path, strip variant): wave k of the grid takes tile_order[k] -- the tiles in descending order
    // of what they cost in the previous frame of this workspace (strip_bin.hip, tile_order_workgroup), so that the long
    // tiles start first and the kernel's tail is made of short ones.  Measured at 2.4 M Gaussians (profiles/r03_a):
    // 146 -> 132 us.  A persistent grid (3 / 4 / 8 waves per SIMD) drawing positions of the same order from a device
    // ticket was also built and measured: 197 - 236 us -- the hardware's workgroup dispatcher refills a slot faster than
    // a resident wave can fetch a ticket, the order entry, the range and the first chunk one after the other.
    auto tile_at = [&](uint32_t li) {  // wave-uniform
        return li < n_tiles ? (tile_order ? (uint32_t)__builtin_amdgcn_readfirstlane(tile_order[li]) : li) : n_tiles;
    };
    auto next_index = [&](uint32_t li) { return li + gridDim.x; };
    uint32_t li = blockIdx.x, nli = next_index(li);
    uint32_t tile = tile_at(li), ntile = tile_at(nli), start, n, nstart, nn;
    range_of(tile, start, n);
    range_of(ntile, nstart, nn);

    // register stage for the next chunk (one Gaussian per lane)
    GaussianRec g;
    float r0 = 0, r1 = 0, r2 = 0;
    float4 cq = make_float4(0.f, 0.f, 0.f, 0.f);
    float dz = 0.f;  // AUX: the Gaussian's depth |p_c| (rec_geom.z, the sort key)
    uint32_t gid = 0, gj = 0;
    bool have = false;
    auto fetch = [&](uint32_t s0, uint32_t cnt, uint32_t base) {
        have = base + lane < cnt;
        if (have) {
            gj = s0 + base + lane;
            gid = raster_load<FRAME>(S, gj, g);
            if (FRAME) cq = S.conic4[(size_t)gid * GS_REC_STRIDE];
            if constexpr (AUX) dz = S.geom[(size_t)gid * GS_REC_STRIDE].z;
            if (CDIM == 3) raster_load_rgb<FRAME>(S, gj, gid, r0, r1, r2);
        }
    };
    fetch(start, n, 0);
    int k = 0;  // chunk counter across tiles: LDS ring slot

    for (; li < n_tiles; li = nli, nli = next_index(nli), tile = ntile, ntile = tile_at(nli), start = nstart, n = nn,
                         range_of(ntile, nstart, nn)) {
        const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
        const uint32_t id_x = tx * 16 + (lane & 15), id_y0 = ty * 16 + (lane >> 4);
        const float px = raster_pixel_coord(id_x, G.padW, G.focal_x);
        f2 py2[NPP];
#pragma unroll
        for (int h = 0; h < NPP; ++h)
            py2[h] = f2{raster_pixel_coord(id_y0 + 8 * h, G.padH, G.focal_y),
                        raster_pixel_coord(id_y0 + 8 * h + 4, G.padH, G.focal_y)};
        constexpr int NB = CDIM > 3 ? CDIM / 3 : 1;  // SH basis functions per channel
        f2 SH[NPP][NB];
        if (CDIM > 3) {
#pragma unroll
            for (int h = 0; h < NPP; ++h) {
                float a9[NB], b9[NB];
                raster_pixel_sh<NB>(id_x, id_y0 + 8 * h, G, a9);
                raster_pixel_sh<NB>(id_x, id_y0 + 8 * h + 4, G, b9);
                constexpr float KS = -GS_LOG2E;  // raster_common.h
#pragma unroll
                for (int k9 = 0; k9 < NB; ++k9) SH[h][k9] = f2{KS * a9[k9], KS * b9[k9]};
            }
        }

        // pair h holds rows y0 + 8h (x) and y0 + 8h + 4 (y): tile pixel indices 128h + lane, 128h + 64 + lane.
        // T is the MASKED transmittance: it drops to exactly 0 once the pixel's transmittance is <= 0.0001
        // (the reference's per-pixel `accum < 0.0001` stop, gaussian.cu:906), so a finished pixel adds nothing.
        f2 T[NPP], cr[NPP], cg[NPP], cb[NPP], accw[NPP];
#pragma unroll
        for (int h = 0; h < NPP; ++h) {
            T[h] = f2{1.0f, 1.0f};
            cr[h] = cg[h] = cb[h] = accw[h] = f2{0.f, 0.f};
        }
        f2 cd[AUX ? NPP : 1], ca[AUX ? NPP : 1];  // AUX: sum w d, sum w
        if constexpr (AUX) {
#pragma unroll
            for (int h = 0; h < NPP; ++h) cd[h] = ca[h] = f2{0.f, 0.f};
        }
        f2 live_scale = splat(GS_LIVE_SCALE), live_bias = splat(-GS_T_STOP * GS_LIVE_SCALE);
        // opaque to the compiler: otherwise it keeps the two constants in SGPRs and copies them into VGPR pairs for the
        // inline v_pk_fma inside the hot loop (two v_mov_b64 per four Gaussians)
        asm volatile("" : "+v"(live_scale), "+v"(live_bias));
        uint32_t nproc = 0, steps = 0;  // steps: Gaussians composited before the wave stopped (the tile's cost)

        // One finished pixel: weight normalisation, padded image, clamp + centred crop.  The epilogue's statement; the compact
        // phase writes a pixel that has stopped when it hands the live ones over, and its own two per lane at the end.
        auto write_pixel = [&](uint32_t id_xp, uint32_t id_y, float c0, float c1, float c2, float aw) {
            if (!WN || aw < 0.01f) aw = 1.0f;  // gaussian.cu:964-969
            fwd_store_pixel(G, out_padded, out_image, id_xp, id_y, c0 / aw, c1 / aw, c2 / aw);
        };

        // COMPACT (rgb inference frames).  A wave composites all 256 pixels of its tile until the last of them stops, and the last
        // one is typically a ray through a gap: a quarter of a frame's steps run with at most half of the pixel slots alive.  At the
        // first liveness test that finds at most KCAP = 128 pixels alive, with at least `compact_min` Gaussians of the list left,
        // the wave COMPACTS: a pixel that has stopped is final -- the masked T is 0, so nothing is ever added to it again -- and is
        // written to the image there and then; the live ones go to s_cmp, ranked in the fixed order of their tile index (ballot
        // masks + mbcnt), and lane L takes entries L and L + 64.  From there on a step is ONE pixel pair per lane instead of two:
        // the same expressions in the same order on the same operands, only dx, B dx and A dx^2 + nlop are per pixel now (three
        // more packed instructions per pair).  T[0], cr[0], cg[0], cb[0] are the pair's state; px2 / py2c its coordinates -- the
        // floats the full phase held, not recomputed; cidx the two tile indices (0xffff: no pixel, T = 0).
        // `vote`: the full phase stops on a LANE's sum of four T, so a pixel whose T is NaN (suspicious chunks only) silences the
        // three other pixels of its lane in the vote.  The compact phase votes per pixel and keeps that rule: vote is 0 for every
        // pixel whose lane of the full layout holds a NaN, refreshed where a NaN can appear (suspicious chunks, `seen_legacy`).
        bool compacted = false, seen_legacy = false;  // (wave-uniform)
        uint32_t compact_at = 0xffffffffu;
        // the kernel sits at its 128 VGPRs: the compact phase's per-lane values live in the registers of the pair it gave up
        f2 &vote = T[1], &px2 = cg[1], &py2c = cb[1];
        auto cidx = [&]() { return __float_as_uint(cr[1].x); };
        auto refresh_vote = [&]() {
            if constexpr (COMPACT) {
                // flags[l] = 1: lane l of the full layout holds a pixel whose T is NaN (the hand-over area is free by now)
                uint32_t l = lane;
                asm volatile("" : "+v"(l));  // (not to be moved: see hand_over)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                s_cmp[KT][l] = 0.f;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (T[0].x != T[0].x) s_cmp[KT][cidx() & 63u] = 1.f;
                if (T[0].y != T[0].y) s_cmp[KT][(cidx() >> 16) & 63u] = 1.f;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                vote.x = 1.0f - s_cmp[KT][cidx() & 63u];
                vote.y = 1.0f - s_cmp[KT][(cidx() >> 16) & 63u];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        };
        // a pixel votes if T x vote > 0; v_max ignores a NaN operand (a NaN pixel's own vote is 0, and NaN x 0 = NaN)
        auto compact_live = [&](bool refresh) {
            if (refresh) refresh_vote();
            const f2 s = T[0] * vote;
            return __ballot(__builtin_fmaxf(s.x, s.y) > 0.0f) != 0ull;
        };

        auto write_ckpt = [&](uint32_t idx_in_tile) {
            float4 *c = ckpt + raster_ckpt_slot(start, tile, idx_in_tile / GS_BUCKET) * 256;
#pragma unroll
            for (int h = 0; h < NPP; ++h) {
                c[128 * h + lane] = make_float4(T[h].x, cr[h].x, cg[h].x, cb[h].x);
                c[128 * h + 64 + lane] = make_float4(T[h].y, cr[h].y, cg[h].y, cb[h].y);
            }
            if constexpr (AUX) {
                float2 *a = X.ckpt + raster_ckpt_slot(start, tile, idx_in_tile / GS_BUCKET) * 256;
#pragma unroll
                for (int h = 0; h < NPP; ++h) {
                    a[128 * h + lane] = make_float2(cd[h].x, ca[h].x);
                    a[128 * h + 64 + lane] = make_float2(cd[h].y, ca[h].y);
                }
            }
        };
        auto any_live = [&]() {
            f2 sum = T[0];
#pragma unroll
            for (int h = 1; h < NPP; ++h) sum += T[h];
            return __ballot(sum.x + sum.y > 0.0f) != 0ull;
        };
        // the hand-over: m[2 h + e] = the lanes whose pixel (h, e) is alive (T != 0: a NaN is carried along), live <= KCAP
        auto hand_over = [&](const unsigned long long (&m)[4]) {
            if constexpr (COMPACT) {
                uint32_t first = 0;
                // opaque, and not to be moved: the four pixels' addresses are per-tile values, and hoisted out of the chunk loop
                // they would sit in registers (or scratch) through the hot loops for a use that comes once per tile
                uint32_t x_here = id_x, y_here = id_y0, l = lane;
                asm volatile("" : "+v"(x_here), "+v"(y_here), "+v"(l));
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int h = q >> 1;
                    const bool e = q & 1;
                    const float t = e ? T[h].y : T[h].x, c0 = e ? cr[h].y : cr[h].x, c1 = e ? cg[h].y : cg[h].x,
                                c2 = e ? cb[h].y : cb[h].x;
                    const uint32_t slot = first + __builtin_amdgcn_mbcnt_hi((uint32_t)(m[q] >> 32),
                                                                            __builtin_amdgcn_mbcnt_lo((uint32_t)m[q], 0u));
                    if (t != 0.f) {  // (the lane's bit of m[q]) slot < live <= KCAP
                        s_cmp[KT][slot] = t;
                        s_cmp[KR][slot] = c0;
                        s_cmp[KG][slot] = c1;
                        s_cmp[KB][slot] = c2;
                        s_cmp[KX][slot] = px;
                        s_cmp[KY][slot] = e ? py2[h].y : py2[h].x;
                        s_cmp[KI][slot] = __uint_as_float(64u * q + l);
                    } else {
                        write_pixel(x_here, y_here + 4 * q, c0, c1, c2, 1.0f);  // stopped: final
                    }
                    first += (uint32_t)__popcll(m[q]);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const uint32_t live = first;
                const bool a = l < live, b = l + 64u < live;
                T[0] = f2{a ? s_cmp[KT][l] : 0.f, b ? s_cmp[KT][l + 64] : 0.f};
                cr[0] = f2{a ? s_cmp[KR][l] : 0.f, b ? s_cmp[KR][l + 64] : 0.f};
                cg[0] = f2{a ? s_cmp[KG][l] : 0.f, b ? s_cmp[KG][l + 64] : 0.f};
                cb[0] = f2{a ? s_cmp[KB][l] : 0.f, b ? s_cmp[KB][l + 64] : 0.f};
                px2 = f2{a ? s_cmp[KX][l] : 0.f, b ? s_cmp[KX][l + 64] : 0.f};
                py2c = f2{a ? s_cmp[KY][l] : 0.f, b ? s_cmp[KY][l + 64] : 0.f};
                cr[1] = f2{__uint_as_float((a ? __float_as_uint(s_cmp[KI][l]) : 0xffffu) |
                                           ((b ? __float_as_uint(s_cmp[KI][l + 64]) : 0xffffu) << 16)), 0.f};
                vote = f2{1.f, 1.f};
                if (seen_legacy) refresh_vote();
            }
        };

        bool done = false, staged_next = false;  // staged_next: the register stage holds chunk 0 of the NEXT tile
        bool continues = false;  // dense frames: the rest of a long list goes to the segment kernels (below)
        for (uint32_t base = 0; base < n && !done; base += CH, ++k) {
            if (FRAME && cont_flag && base == (uint32_t)GS_LONG_MIN) {  // uniform
                if (any_live()) {
                    // still alive after GS_LONG_MIN Gaussians (low-opacity pile-ups: a list of 100,000 would keep this
                    // ONE wave busy for milliseconds): the pixels' state is saved and the rest of the list is composited in
                    // segments by many waves (raster_segment_kernel); lists that saturate earlier never get here
                    float4 *c = cont_state + (size_t)tile * 256;
                    uint32_t l = lane;
                    // (COMPACT: the kernel has no register to spare for a lane's address that is used once in a dense frame's tile)
                    if constexpr (COMPACT) asm volatile("" : "+v"(l));
#pragma unroll
                    for (int h = 0; h < NPP; ++h) {
                        c[128 * h + l] = make_float4(T[h].x, cr[h].x, cg[h].x, cb[h].x);
                        c[128 * h + 64 + l] = make_float4(T[h].y, cr[h].y, cg[h].y, cb[h].y);
                    }
                    continues = true;
                }
                if (continues) break;
            }
            const int buf = k & (SM::NBUF - 1);  // no SH: two-deep ring (the wave is in program order, so writing buffer
                                                 // k & 1 here cannot overtake its own reads of two chunks ago)
            // Can a Gaussian of this chunk yield a non-finite alpha (or colour) for some pixel?  Not if its record is
            // finite and its conic positive semi-definite and of ordinary size: then q >= -(rounding of a few hundred) and
            // alpha = 2^-(q + nlop) stays finite (|dx|, |dy| < 4: visible Gaussians lie inside the guard band).  Only chunks
            // with a Gaussian that fails the test need the DX9 multiply below (wave-uniform: one ballot per 64 Gaussians).
            bool suspicious = false;
            if (have) {
                float A, B, C;
                if (FRAME) {  // S1 stored the conic in the Gaussian's record (same line as geom / colour)
                    A = cq.x;
                    B = cq.y;
                    C = cq.z;
                } else {
                    raster_conic(g, A, B, C);
                }
                {
                    const float chk = ((g.x + g.y) + (A + B + C)) + ((r0 + r1 + r2) + g.opa);  // NaN / inf propagate
                    suspicious = !(fabsf(chk) < 3.0e38f) || !(A >= 0.f && A < 1.0e8f) || !(C >= 0.f && C < 1.0e8f) ||
                                 !(4.f * A * C >= B * B) ||
                                 !FRAME || CDIM != 3;
                }
                float opa = g.opa;
                if (SIG)  // gaussian.cu:918: (1.0/2*3.1415926536) * rsqrtf(det + 1e-7), folded into opacity
                    opa *= 1.5707963268f * rsqrtf(raster_det(g.a, g.b, g.c, g.d) + 1e-7f);
                sm.f[buf][SM::X][lane] = g.x;
                sm.f[buf][SM::Y][lane] = g.y;
                if constexpr (EXACT) {
                    // gaussian.cu:916-923: the exponent's argument is a float numerator over the DOUBLE 2 det + 1e-14
                    const double den = (double)(2.0f * raster_det(g.a, g.b, g.c, g.d)) + 1e-14;
                    const float dh = (float)den;
                    sm.f[buf][SM::A][lane] = g.a;
                    sm.f[buf][SM::B][lane] = g.b + g.c;
                    sm.f[buf][SM::C][lane] = g.d;
                    sm.f[buf][SM::DH][lane] = dh;
                    sm.f[buf][SM::DL][lane] = (float)(den - (double)dh);
                } else {
                    sm.f[buf][SM::A][lane] = A;
                    sm.f[buf][SM::B][lane] = B;
                    sm.f[buf][SM::C][lane] = C;
                }
                // frame path: the opacity (a sigmoid, > 0) rides in the exponent, alpha = 2^-(q + nlop); the
                // reference API may be handed any opacity (zero, negative), so it keeps the multiplication
                sm.f[buf][SM::NLOP][lane] = FRAME ? -__log2f(opa) : opa;
                if constexpr (AUX) s_dep[buf][lane] = dz;
                if constexpr (CDIM == 3) {
                    fwd_confine_nan_colour(r0, r1, r2, sm.f[buf][SM::NLOP][lane]);
                    sm.f[buf][SM::R][lane] = r0;
                    sm.f[buf][SM::G][lane] = r1;
                    sm.f[buf][SM::BL][lane] = r2;
                } else {
                    const float *src = raster_sh_ptr<FRAME, CDIM>(S, gj, gid);
#pragma unroll
                    for (int q = 0; q < CDIM; ++q) sm.sh[buf][lane][q] = src[q];
                }
            } else if (base + lane < ((n + (GROUP - 1u)) & ~(GROUP - 1u))) {
                // pad the ragged tail to a multiple of GROUP with null Gaussians (opacity 0 => alpha 0)
#pragma unroll
                for (int q = 0; q < SM::NFIELD; ++q)  // (exact flavour: denominator 1, so that the null Gaussian's alpha is 0 x exp(0))
                    sm.f[buf][q][lane] = (FRAME && q == SM::NLOP) ? 1e30f : (EXACT && q == SM::DH) ? 1.0f : 0.f;
                if constexpr (AUX) s_dep[buf][lane] = 0.f;
                if constexpr (CDIM > 3) {
#pragma unroll
                    for (int q = 0; q < CDIM; ++q) sm.sh[buf][lane][q] = 0.f;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // overlaps with the compositing below: the next chunk of this tile, or chunk 0 of the next tile
            staged_next = base + CH >= n;
            if (staged_next)
                fetch(nstart, nn, 0);
            else
                fetch(start, n, base + CH);
            const uint32_t cnt = (n - base) < (uint32_t)CH ? (n - base) : (uint32_t)CH;
            // CH == GS_BUCKET: one checkpoint per chunk; the state before the tile's first chunk is (T, C) = (1, 0) by
            // definition, the backward kernels synthesise it instead of reading 4 KiB per tile back
            if (CKPT && base > 0) write_ckpt(base);
            // groups of GROUP Gaussians: a wave-uniform liveness test every LIVE_EVERY Gaussians, per-pixel masking inside
            // (exactly the reference's per-pixel `accum < 0.0001` test, gaussian.cu:906)
            const bool chunk_legacy = __ballot(suspicious) != 0ull;
            auto composite_chunk = [&](auto legacy_tag) {
                constexpr bool LEGACY = decltype(legacy_tag)::value;
                uint32_t stop = cnt;  // Gaussians of this chunk composited before the wave stopped
                uint32_t i = 0;
                bool hand = false;  // (uniform) the full loop has just asked for the hand-over
                if (!COMPACT || !compacted) {
#pragma unroll 1
                    for (; i < cnt; i += GROUP) {
                        if ((i & (LIVE_EVERY - 1)) == 0) {
                            if (!any_live()) {
                                done = true;
                                stop = i;
                                break;
                            }
                            if constexpr (COMPACT) {
                                // (compact_min = 0: switched off, or a dense frame -- its hand-over at GS_LONG_MIN stores the fixed layout)
                                // only the COUNT of live pixels (T != 0: a NaN is carried along) is taken inside the loop: four v_cmp into
                                // SGPR masks and s_bcnt1.  The hand-over itself stands behind the loop, so that nothing of it is live here.
                                if (compact_min && n - (base + i) >= compact_min &&
                                    __popcll(__ballot(T[0].x != 0.f)) + __popcll(__ballot(T[0].y != 0.f)) + __popcll(__ballot(T[1].x != 0.f)) +
                                            __popcll(__ballot(T[1].y != 0.f)) <= KCAP) {
                                    compacted = hand = true;
                                    compact_at = base + i;
                                    break;
                                }
                            }
                        }
                        {
                            constexpr uint32_t i4 = 0;
                            struct Vg {
                                float v[GROUP];
                            };
                            auto ld4 = [&](int q) {
                                Vg r;
                                if constexpr (GROUP == 4) {
                                    const float4 t = *(const float4 *)__builtin_assume_aligned(&sm.f[buf][q][i + i4], 16);
                                    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
                                } else {
                                    const float2 t = *(const float2 *)__builtin_assume_aligned(&sm.f[buf][q][i + i4], 8);
                                    r.v[0] = t.x; r.v[1] = t.y;
                                }
                                return r;
                            };
                            const Vg X = ld4(SM::X), Y = ld4(SM::Y), A4 = ld4(SM::A), B4 = ld4(SM::B), C4 = ld4(SM::C);
                            const Vg O4 = ld4(SM::NLOP);
                            Vg DH4 = {}, DL4 = {};
                            if constexpr (EXACT) {
                                DH4 = ld4(SM::DH);
                                DL4 = ld4(SM::DL);
                            }
                            Vg R4 = {}, G4 = {}, L4 = {}, D4 = {};
                            if constexpr (AUX) {
                                static_assert(GROUP == 4, "AUX: the depths are read four at a time");
                                const float4 t = *(const float4 *)__builtin_assume_aligned(&s_dep[buf][i + i4], 16);
                                D4.v[0] = t.x; D4.v[1] = t.y; D4.v[2] = t.z; D4.v[3] = t.w;
                            }
                            if constexpr (CDIM == 3) {
                                R4 = ld4(SM::R);
                                G4 = ld4(SM::G);
                                L4 = ld4(SM::BL);
                            }
                            f2 fp[NPP], fm[NPP];  // COMPACT: the step before, unmasked, and its liveness mask
#pragma unroll
                            for (int h = 0; h < NPP; ++h) fp[h] = fm[h] = T[h];
#pragma unroll
                            for (int u = 0; u < (int)GROUP; ++u) {
                                const float gx = X.v[u], gy = Y.v[u], cA = A4.v[u], cB = B4.v[u], cC = C4.v[u], nlop = O4.v[u];
                                // q + nlop = (C dy - B dx) dy + (A dx^2 + nlop): dx is shared by the lane's four pixels
                                const float dx = px - gx;
                                const float bdx = cB * dx;
                                const float f = FRAME ? fmaf(cA * dx, dx, nlop) : cA * dx * dx;
#pragma unroll
                                for (int h = 0; h < NPP; ++h) {
                                    const f2 dy = py2[h] - splat(gy);
                                    f2 al;
                                    if constexpr (EXACT) {
                                        // exp(double(-(d x x - (b + c) x y + a y y)) / (2 det + 1e-14)) rounded to float: the reference's
                                        // `fast = 0` flavour (gaussian.cu:922-923), float products in its order (no contraction), then
                                        // the double division and the double exponential it pays per pixel as well
                                        const double den = (double)DH4.v[u] + (double)DL4.v[u];
                                        auto exact_alpha = [&](float y) {
                                            const float t1 = __fmul_rn(__fmul_rn(cC, dx), dx);   // d x x
                                            const float t2 = __fmul_rn(__fmul_rn(cB, dx), y);    // (b + c) x y
                                            const float t3 = __fmul_rn(__fmul_rn(cA, y), y);     // a y y
                                            const float num = -__fadd_rn(__fsub_rn(t1, t2), t3);
                                            return (float)exp((double)num / den);
                                        };
                                        al.x = exact_alpha(dy.x);
                                        al.y = exact_alpha(dy.y);
                                    } else {
                                        const f2 q = pk_fma(pk_fma(splat(cC), dy, splat(-bdx)), dy, splat(f));
                                        al.x = gs_exp2(-q.x);
                                        al.y = gs_exp2(-q.y);
                                    }
                                    if (!FRAME) al = al * splat(nlop);
                                    if (SIG) {  // gaussian.cu:930
                                        al.x = gs_squash_alpha(al.x);
                                        al.y = gs_squash_alpha(al.y);
                                    }
                                    // LEGACY: w = alpha T with 0 x anything = 0 (v_mul_legacy_f32's rule): a finished pixel (T == 0) stays
                                    // untouched whatever alpha is -- NaN, infinite --, like the reference, which `break`s before it
                                    // evaluates the Gaussian (gaussian.cu:906); a live pixel sees the NaN, as there.
                                    // rgb frames take this variant for SOME chunks (`suspicious`, above) and the plain one for the others,
                                    // and which Gaussians share a chunk depends on the list: an occlusion-culled frame's list lacks the pairs
                                    // behind the tile's cut, so a chunk that holds a suspicious Gaussian in the full list need not hold one
                                    // in the trimmed list.  The two variants must therefore round alike on ordinary values -- the culled
                                    // frame is the unculled one bit for bit -- and the intrinsic does not: behind it T - w is a rounded
                                    // product subtracted, behind the plain product the compiler is free to contract.  So there a finished
                                    // pixel's alpha is replaced by 0 and the statements that follow are the plain variant's.
                                    // (Every other instantiation takes this variant for every chunk and keeps the intrinsic.)
                                    f2 w;
                                    if constexpr (COMPACT) {
                                        // The kernel with a compact phase: both phases must round T (1 - alpha) alike, so the step is stated
                                        // with builtins here and there -- the forms the compiler's contraction gave this loop when the
                                        // statements below were left to it (raster_compact_codegen.txt), so that the frame is what it was.
                                        // T of the group's first Gaussian is materialised; behind it T = t' m is the product of the step before
                                        // (fp[h], fm[h]; m = 0 or 1: exact).
                                        const f2 Tn = u == 0 ? T[h] : fp[h] * fm[h];
                                        if constexpr (LEGACY) {
                                            al.x = Tn.x == 0.f ? 0.f : al.x;
                                            al.y = Tn.y == 0.f ? 0.f : al.y;
                                        }
                                        w = Tn * al;
                                    } else if constexpr (LEGACY && FRAME && CDIM == 3) {
                                        al.x = T[h].x == 0.f ? 0.f : al.x;
                                        al.y = T[h].y == 0.f ? 0.f : al.y;
                                        w = al * T[h];
                                    } else if constexpr (LEGACY)
                                        w = f2{mul_legacy(al.x, T[h].x), mul_legacy(al.y, T[h].y)};
                                    else
                                        w = al * T[h];
                                    if constexpr (CDIM == 3) {
                                        cr[h] = pk_fma(splat(R4.v[u]), w, cr[h]);
                                        cg[h] = pk_fma(splat(G4.v[u]), w, cg[h]);
                                        cb[h] = pk_fma(splat(L4.v[u]), w, cb[h]);
                                    } else {
                                        const float *co = sm.sh[buf][i + i4 + u];
                                        f2 v0 = {0.f, 0.f}, v1 = {0.f, 0.f}, v2 = {0.f, 0.f};
#pragma unroll
                                        for (int k9 = 0; k9 < NB; ++k9) {
                                            v0 = pk_fma(SH[h][k9], splat(co[k9]), v0);
                                            v1 = pk_fma(SH[h][k9], splat(co[NB + k9]), v1);
                                            v2 = pk_fma(SH[h][k9], splat(co[2 * NB + k9]), v2);
                                        }
                                        auto sg = [](float v) { return gs_rcp(1.0f + gs_exp2(v)); };
                                        const f2 c0 = {sg(v0.x), sg(v0.y)}, c1 = {sg(v1.x), sg(v1.y)}, c2 = {sg(v2.x), sg(v2.y)};
                                        cr[h] = pk_fma(w, c0, cr[h]);
                                        cg[h] = pk_fma(w, c1, cg[h]);
                                        cb[h] = pk_fma(w, c2, cb[h]);
                                    }
                                    if (WN) accw[h] += w;
                                    if constexpr (AUX) {  // alpha: a colour channel of value 1.0 (fma(1, w, a) == a + w)
                                        cd[h] = pk_fma(splat(D4.v[u]), w, cd[h]);
                                        // w opaque here: otherwise a + alpha x T is contracted into one fma, which rounds differently
                                        // from the colour channels' fma(c, w, C) of the ROUNDED w
                                        f2 wr = w;
                                        asm("" : "+v"(wr));
                                        ca[h] += wr;
                                    }
                                    if constexpr (COMPACT) {
                                        const f2 Tn = u == 0 ? T[h] : fp[h] * fm[h];
                                        const f2 t = u == 0 ? pk_fma(-Tn, al, Tn) : u == 1 ? pk_fma(fp[h], fm[h], -w) : pk_fma(fm[h], fp[h], -w);
                                        fp[h] = t;
                                        fm[h] = live_mask(t, live_scale, live_bias);
                                        if (u == (int)GROUP - 1) T[h] = fp[h] * fm[h];
                                    } else {
                                        const f2 t = T[h] - w;  // T * (1 - alpha)
                                        T[h] = t * live_mask(t, live_scale, live_bias);
                                    }
                                }
                            }
                        }
                    }
                }
                if constexpr (COMPACT) {
                    if (hand) {
                        asm volatile("" : "+v"(T[0]), "+v"(T[1]));  // (the masks are taken again here, not carried out of the loop)
                        const unsigned long long m[4] = {__ballot(T[0].x != 0.f), __ballot(T[0].y != 0.f), __ballot(T[1].x != 0.f),
                                                         __ballot(T[1].y != 0.f)};
                        hand_over(m);
                    }
                    if (compacted && !done) {
                        // the compact loop: eight Gaussians per trip, one liveness test; i is a multiple of LIVE_EVERY here
                        static_assert(GROUP == 4 && LIVE_EVERY == 8, "the compact loop walks two groups of four per liveness test");
                        // (a NaN that appeared behind the last test of a suspicious chunk: the plain loop's tests do not look again)
                        if (!LEGACY && seen_legacy && i == 0) refresh_vote();
#pragma unroll 1
                        for (; i < cnt; i += 2 * GROUP) {
                            if (!compact_live(LEGACY)) {
                                done = true;
                                stop = i;
                                break;
                            }
#pragma unroll
                            for (uint32_t i4 = 0; i4 < 2 * GROUP; i4 += GROUP) {
                                if (i4 && i + i4 >= cnt) break;  // (uniform) the list ends inside the trip
                                // (the second group's nine operand reads stay behind the first group's math: 36 registers)
                                __builtin_amdgcn_sched_barrier(0);
                                auto ld4 = [&](int q) { return *(const float4 *)__builtin_assume_aligned(&sm.f[buf][q][i + i4], 16); };
                                const float4 X = ld4(SM::X), Y = ld4(SM::Y), A4 = ld4(SM::A), B4 = ld4(SM::B), C4 = ld4(SM::C);
                                const float4 O4 = ld4(SM::NLOP), R4 = ld4(SM::R), G4 = ld4(SM::G), L4 = ld4(SM::BL);
                                auto at = [](const float4 &v, int u) { return u == 0 ? v.x : u == 1 ? v.y : u == 2 ? v.z : v.w; };
                                f2 tp = T[0], mk = T[0];  // the step before: T (1 - alpha) unmasked, and its liveness mask
#pragma unroll
                                for (int u = 0; u < (int)GROUP; ++u) {
                                    const float gx = at(X, u), gy = at(Y, u), cA = at(A4, u), cB = at(B4, u), cC = at(C4, u),
                                                nlop = at(O4, u);
                                    // the full loop's expressions, per pixel: every product and sum rounds as it does there
                                    const f2 dx = px2 - splat(gx);
                                    const f2 bdx = splat(cB) * dx;
                                    const f2 f = pk_fma(splat(cA) * dx, dx, splat(nlop));
                                    const f2 dy = py2c - splat(gy);
                                    const f2 q = pk_fma(pk_fma(splat(cC), dy, -bdx), dy, f);
                                    f2 al = {gs_exp2(-q.x), gs_exp2(-q.y)};
                                    // T (1 - alpha) as the full loop's code computes it.  That code is compiled with contraction, and
                                    // what the compiler makes of `T - al * T` there is pinned here by builtins, instruction for
                                    // instruction -- operand roles included, which decide the sign of a NaN: the first Gaussian of a
                                    // group of four takes fma(-T, al, T); for the three others T is the product t' m of the step
                                    // before (m = 0 or 1: exact) and the step is fma(t', m, -w) with the ROUNDED w = T al.
                                    const f2 Tn = u == 0 ? T[0] : tp * mk;
                                    if constexpr (LEGACY) {
                                        al.x = Tn.x == 0.f ? 0.f : al.x;
                                        al.y = Tn.y == 0.f ? 0.f : al.y;
                                    }
                                    const f2 w = Tn * al;
                                    // (the factors' places are the full loop's too: t' m for the second Gaussian, m t' for the last two)
                                    const f2 t = u == 0 ? pk_fma(-Tn, al, Tn) : u == 1 ? pk_fma(tp, mk, -w) : pk_fma(mk, tp, -w);
                                    cr[0] = pk_fma(splat(at(R4, u)), w, cr[0]);
                                    cg[0] = pk_fma(splat(at(G4, u)), w, cg[0]);
                                    cb[0] = pk_fma(splat(at(L4, u)), w, cb[0]);
                                    tp = t;
                                    mk = live_mask(t, live_scale, live_bias);
                                }
                                T[0] = tp * mk;
                            }
                        }
                    }
                }
                return stop;
            };
            if constexpr (COMPACT) seen_legacy = seen_legacy || chunk_legacy;
            steps = base + (chunk_legacy ? composite_chunk(std::true_type{}) : composite_chunk(std::false_type{}));
            // a chunk whose checkpoint was written counts as processed even if the wave stopped inside it:
            // the backward pass masks finished pixels by their transmittance
            nproc = base + cnt;
        }
        if (!staged_next) fetch(nstart, nn, 0);  // empty tile, or the wave stopped before its last chunk
        if (FRAME && !CKPT && cut_out) {  // (uniform; inference frames only: the training variant sits at its 128-VGPR budget)
            // all pixels stopped inside the list (or exactly at its end): nothing behind the last composited Gaussian matters
            const bool sat = !continues && steps > 0 && (done || !((COMPACT && compacted) ? compact_live(seen_legacy) : any_live()));
            if (lane == 0) {
                uint32_t c = GS_NO_CUT, dlast = GS_NO_CUT;
                if (sat) {
                    const uint32_t last = S.ids[start + steps - 1];
                    const float zl = S.geom[(size_t)last * GS_REC_STRIDE].z;  // the depth bits the trim compared (rects[].z)
                    dlast = __float_as_uint(zl);
                    c = __float_as_uint(zl * (1.0f + GS_CUT_MARGIN));
                }
                // A trimmed list (this tile had a cut) is every pair up to the cut plus SOME of the deeper ones (gs_frame_layout.h):
                // only a walk that ended inside {d <= cut} with every pixel stopped saw what the full list would have shown it.
                // The list ascends in depth, so the last composited pair decides.  (cut_in may be cut_out: read before the store)
                if (cut_in) {
                    const uint32_t ci = cut_in[tile];
                    unsigned long long one = 1ull;
                    if constexpr (COMPACT) asm volatile("" : "+v"(one));  // (as above: not a constant kept in two registers)
                    if (ci != GS_NO_CUT && dlast > ci) *ranpast = one;  // (!sat: dlast = GS_NO_CUT, the largest value there is)
                }
                cut_out[tile] = c;
            }
        }
        if (tile_nproc && lane == 0) tile_nproc[tile] = nproc;
        if (FRAME && tile_cost && lane == 0) tile_cost[tile] = steps;
        // statistics for the caller's long-list cost model (gs_frame.py): the longest walk a wave actually made -- a list's
        // LENGTH says nothing about a tile whose pixels stop early -- and the steps beyond the first GS_LONG_MIN of every walk
        // (what the segmented compositing would take over).  Rare (tiles beyond 512 / 1,024 steps), so the atomics cost nothing.
        if (FRAME && ranpast && lane == 0 && steps > (uint32_t)GS_LONG_MIN) {
            atomicAdd(ranpast + (GS_CNT_EXCESS_WALK - GS_CNT_RANPAST), (unsigned long long)(steps - (uint32_t)GS_LONG_MIN));
            if (steps > (uint32_t)GS_LONGEST_MIN) atomicMax(ranpast + (GS_CNT_MAXWALK - GS_CNT_RANPAST), (unsigned long long)steps);
        }
        if (FRAME && cont_flag && lane == 0) cont_flag[tile] = continues ? 1u : 0u;
        if constexpr (COMPACT) {  // the step at which the tile compacted (gs_frame_debug_tile_compact)
            if (lane == 0) tile_compact[tile] = compact_at;  // (never null for this instantiation: gs_stage_raster_forward)
        }

        if (COMPACT && compacted) {  // (uniform) each lane's up to two pixels, by their index in the tile
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const uint32_t p = (cidx() >> (16 * e)) & 0xffffu;
                if (p != 0xffffu)
                    write_pixel(tx * 16 + (p & 15u), ty * 16 + ((p >> 4) & 3u) + 4 * (p >> 6), e ? cr[0].y : cr[0].x,
                                e ? cg[0].y : cg[0].x, e ? cb[0].y : cb[0].x, 1.0f);
            }
        } else {
#pragma unroll
            for (int h = 0; h < NPP; ++h)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const uint32_t id_y = id_y0 + 8 * h + 4 * e;
                    if constexpr (AUX) {
                        const float dv = e ? cd[h].y : cd[h].x, av = e ? ca[h].y : ca[h].x;
                        if (X.padded) X.padded[(size_t)id_y * G.padW + id_x] = make_float2(dv, av);
                        const int ox = (int)id_x - G.crop_left, oy = (int)id_y - G.crop_top;
                        if (ox >= 0 && ox < G.width && oy >= 0 && oy < G.height) {  // cropped like the image, not clamped
                            if (X.depth) X.depth[(size_t)oy * G.width + ox] = dv;
                            if (X.alpha) X.alpha[(size_t)oy * G.width + ox] = av;
                        }
                    }
                    write_pixel(id_x, id_y, e ? cr[h].y : cr[h].x, e ? cg[h].y : cg[h].x, e ? cb[h].y : cb[h].x,
                                e ? accw[h].y : accw[h].x);
                }
        }
    }  // tile loop
}

template <int CDIM, bool FRAME, bool CKPT, bool SIG, bool WN, bool EXACT = false>
__global__ void __launch_bounds__(FWD_THREADS)
__attribute__((amdgpu_waves_per_eu(CDIM == 48 ? GS_FWD_SH48_WPE : CDIM == 27 ? GS_FWD_SH27_WPE
                                               : (SIG || WN || EXACT) ? 1 : GS_FWD_RGB_WPE)))  // (the rare flags would spill at 128)
raster_forward_kernel(RasterSrc S, RasterGeom G, const int32_t *__restrict__ ranges, float *__restrict__ out_padded,
                      float *__restrict__ out_image, float4 *__restrict__ ckpt, uint32_t *__restrict__ tile_nproc,
                      uint32_t n_tiles, float4 *__restrict__ cont_state, uint32_t *__restrict__ cont_flag,
                      const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost, const uint32_t *cut_in,
                      uint32_t *cut_out, unsigned long long *__restrict__ ranpast,
                      const unsigned long long *__restrict__ gate, uint32_t compact_min,
                      uint32_t *__restrict__ tile_compact) {
    // the compact phase: the rgb inference frame only (compact_min = 0 switches it off: GS_FWD_COMPACT=0)
    constexpr bool COMPACT = CDIM == 3 && FRAME && !CKPT && !SIG && !WN && !EXACT;
    raster_forward_body<CDIM, FRAME, CKPT, SIG, WN, EXACT, false, COMPACT>(S, G, ranges, out_padded, out_image, ckpt,
                                                                           tile_nproc, n_tiles, cont_state, cont_flag,
                                                                           tile_order, tile_cost, cut_in, cut_out, ranpast,
                                                                           gate, AuxFwdOut{}, compact_min, tile_compact);
}

// GS_FRAME_AUX frames (frame path only): the compositing with the depth and alpha maps.  No segmented compositing of long
// lists (the frame walks every list with one wave, as GS_FRAME_SERIAL_LONG_LISTS frames do).  Register budget: the four
// accumulators and the staged depth do not fit the rgb kernel's 128 VGPRs -- three waves per SIMD (budgets:
// tests/test_aux_host.py).
#ifndef GS_FWD_AUX_RGB_WPE
#define GS_FWD_AUX_RGB_WPE 3
#endif
#ifndef GS_FWD_AUX_SH27_WPE
#define GS_FWD_AUX_SH27_WPE GS_FWD_SH27_WPE
#endif
template <int CDIM, bool CKPT>
__global__ void __launch_bounds__(FWD_THREADS)
__attribute__((amdgpu_waves_per_eu(CDIM == 48 ? GS_FWD_SH48_WPE : CDIM == 27 ? GS_FWD_AUX_SH27_WPE : GS_FWD_AUX_RGB_WPE)))
raster_aux_forward_kernel(RasterSrc S, RasterGeom G, const int32_t *__restrict__ ranges, float *__restrict__ out_padded,
                          float *__restrict__ out_image, float4 *__restrict__ ckpt, uint32_t *__restrict__ tile_nproc,
                          uint32_t n_tiles, const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost,
                          const uint32_t *cut_in, uint32_t *cut_out, unsigned long long *__restrict__ ranpast,
                          const unsigned long long *__restrict__ gate, AuxFwdOut X) {
    raster_forward_body<CDIM, true, CKPT, false, false, false, true>(S, G, ranges, out_padded, out_image, ckpt, tile_nproc,
                                                                     n_tiles, nullptr, nullptr, tile_order, tile_cost,
                                                                     cut_in, cut_out, ranpast, gate, X);
}

template <int CDIM, bool FRAME, bool CKPT, bool SIG, bool EXACT = false>
void launch_fwd(const RasterSrc &S, const RasterGeom &G, const int32_t *ranges, float *out_padded, float *out_image,
                float4 *ckpt, uint32_t *tile_nproc, int wn, hipStream_t stream, float4 *cont_state = nullptr,
                uint32_t *cont_flag = nullptr, const uint32_t *tile_order = nullptr, uint32_t *tile_cost = nullptr,
                const uint32_t *cut_in = nullptr, uint32_t *cut_out = nullptr, unsigned long long *ranpast = nullptr,
                const unsigned long long *gate = nullptr, uint32_t compact_min = 0, uint32_t *tile_compact = nullptr) {
    tile_order = fwd_tile_order(tile_order);
    const uint32_t T = (uint32_t)(G.ntx * G.nty);
    const uint32_t grid = fwd_launch_grid(T, gate);
    if (wn)
        hipLaunchKernelGGL((raster_forward_kernel<CDIM, FRAME, CKPT, SIG, true, EXACT>), dim3(grid), dim3(FWD_THREADS),
                           0, stream, S, G, ranges, out_padded, out_image, ckpt, tile_nproc, T, cont_state, cont_flag,
                           tile_order, tile_cost, cut_in, cut_out, ranpast, gate, compact_min, tile_compact);
    else
        hipLaunchKernelGGL((raster_forward_kernel<CDIM, FRAME, CKPT, SIG, false, EXACT>), dim3(grid), dim3(FWD_THREADS),
                           0, stream, S, G, ranges, out_padded, out_image, ckpt, tile_nproc, T, cont_state, cont_flag,
                           tile_order, tile_cost, cut_in, cut_out, ranpast, gate, compact_min, tile_compact);
}

}  // namespace
