// track_gate.hip -- gs_loss_track_gated (include/gs_abi.h): the tracking loss of map_loss.hip with each term gated at a
// multiple of the frame's own median residual -- the outlier rule of SplaTAM -- decided on the device.
//
// Per pixel, with the expressions of track_loss_pixel (map_loss.hip; map_terms.h):  covered = A >= alpha_min,
//   c = (|d0| + |d1|) + |d2|  (d = I - T),   a = |D / A - z|.
// S_d = covered, measured, a <= FLT_MAX;  S_c = covered, c <= FLT_MAX;  m_d, m_c: the LOWER medians (rank (n - 1) / 2, an
// element of the set; 0 for an empty set), taken before any gating;  t = max(fl(k m), floor).  A term counts where its
// residual is <= t (k <= 0: the term's gate is off and the rule is gs_loss_track's); with `couple` a pixel of S_d that fails
// the depth gate loses its colour term too.
//
// A non-negative float orders like its bit pattern, so the median is an exact radix select over 10 + 11 + 10 bits:
//   1  hipMemsetAsync            the three levels' counters (48 KiB)
//   2  track_gate_residual_kernel  streams I, T, D, A, z (44 B / pixel) once, stores a and c (NaN outside the sets: 8 B /
//                                pixel, all the later passes read), counts bits 30..21 of both patterns
//   3  track_gate_digit_kernel<1>  every workgroup finds the level-0 bin that holds the rank (track_gate_select: 2 x 2,048
//                                counters from L2, one workgroup scan), then counts bits 20..10 of the elements in that bin
//                                (about 128 workgroups: see TG_DIGIT_BLOCKS)
//   4  track_gate_digit_kernel<2>  the same one level down: bits 9..0 of the elements that match the 21-bit prefix
//   5  track_gate_loss_kernel      the last select gives both medians' bits; thresholds; the five gradient maps and one row of
//                                sums per workgroup, in track_loss_kernel's order
//   6  track_gate_finalize_kernel  the rows in double, in track_loss_finalize_kernel's order
// Both medians travel through the same launches.  The select is redone by every workgroup instead of in a one-workgroup
// launch of its own between the passes: 16 KiB of L2 reads and one 256-thread scan per workgroup against ~2 launches' latency
// per level -- at 640 x 480 the whole chain is launch latency.  Counting is integer: LDS atomics per workgroup (a bin holds at
// most the workgroup's pixels, < 2^32), then one global atomic add per non-empty bin into 32-bit counters (a bin holds at most H W <=
// 2^24).  Integer addition does not depend on order: bitwise repeatable.  No float atomics, no host synchronisation; the
// thresholds never leave the device.
#include <cmath>

#include "gs_common.h"
#include "map_terms.h"

namespace {

constexpr int TG_BLOCK = 256, TG_PER_BLOCK = TG_BLOCK * 4;  // a chunk: track_loss_kernel's geometry, 1,024 pixels
// A counting workgroup ends with one global add per non-empty bin, and adds to one address serialise: the counting passes give
// a workgroup several chunks so that few workgroups flush -- the residual pass (which streams 52 bytes per pixel and wants
// the whole chip) at most about 512 of them, the digit passes (8 bytes per pixel) about 128.
constexpr int TG_RESIDUAL_BLOCKS = 512, TG_RESIDUAL_MAX_CHUNKS = 8, TG_DIGIT_BLOCKS = 128;
constexpr int TG_BINS = 2048, TG_LEVELS = 3;
constexpr float TG_FLT_MAX = 3.402823466e38f;
constexpr int64_t TG_MAX_PIXELS = (int64_t)1 << 24;  // the counts come back as floats

// the state words the passes hand on (uint32; [10..13] hold floats)
enum { TG_BIN0_D, TG_RANK1_D, TG_BIN0_C, TG_RANK1_C, TG_N_D, TG_N_C, TG_BIN1_D, TG_RANK2_D, TG_BIN1_C, TG_RANK2_C, TG_M_D, TG_M_C,
       TG_T_D, TG_T_C, TG_STATE_WORDS = 64 };

inline int64_t tg_blocks(int64_t n) { return (n + TG_PER_BLOCK - 1) / TG_PER_BLOCK; }

struct tg_layout {
    size_t part, hist, state, resid_a, resid_c, total;
};
inline tg_layout tg_workspace(int64_t n) {
    tg_layout L;
    size_t o = 0;
    L.part = o, o += gs_align_up(sizeof(float4) * (size_t)tg_blocks(n), 256);
    L.hist = o, o += sizeof(uint32_t) * TG_LEVELS * 2 * TG_BINS;
    L.state = o, o += sizeof(uint32_t) * TG_STATE_WORDS;
    L.resid_a = o, o += gs_align_up(sizeof(float) * (size_t)n, 256);
    L.resid_c = o, o += gs_align_up(sizeof(float) * (size_t)n, 256);
    L.total = o;
    return L;
}

// the digit of level L of a residual's bit pattern (the sign bit is clear: level 0 has 10 bits)
template <int L>
__device__ __forceinline__ uint32_t tg_digit(uint32_t key) {
    return L == 0 ? (key >> 21) & 2047u : (L == 1 ? (key >> 10) & 2047u : key & 1023u);
}

// count one residual of a set (v <= FLT_MAX: false for the NaN that marks "outside") whose bits above level L are `prefix`
template <int L>
__device__ __forceinline__ void tg_count(float v, uint32_t prefix, uint32_t *s_h) {
    if (!(v <= TG_FLT_MAX)) return;
    const uint32_t key = __float_as_uint(v);
    if (L == 1 && (key >> 21) != prefix) return;
    if (L == 2 && (key >> 10) != prefix) return;
    atomicAdd(&s_h[tg_digit<L>(key)], 1u);
}

__device__ __forceinline__ void tg_zero_lds(uint32_t *s_h) {
    for (int j = threadIdx.x; j < 2 * TG_BINS; j += TG_BLOCK) s_h[j] = 0u;
}
__device__ __forceinline__ void tg_flush_lds(const uint32_t *s_h, uint32_t *__restrict__ hist) {
    for (int j = threadIdx.x; j < 2 * TG_BINS; j += TG_BLOCK) {
        const uint32_t v = s_h[j];
        if (v) atomicAdd(&hist[j], v);
    }
}

struct tg_pick {
    uint32_t bin[2], rank[2], total[2];
};

// For both sets at once: the bin of hist[set][0..2047] that holds the element of rank `rank[set]` (counting from 0) and that
// element's rank inside the bin; MEDIAN: the rank is (total - 1) / 2 of the level's own total.  An empty level gives bin 0,
// rank 0.  Called by all 256 threads; thread t owns bins 8t .. 8t + 7.  Ends with a barrier.
template <bool MEDIAN>
__device__ __forceinline__ tg_pick track_gate_select(const uint32_t *__restrict__ hist, uint32_t rank_d, uint32_t rank_c) {
    __shared__ uint32_t s_wt[2][TG_BLOCK / 64], s_res[2][2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t b[2][8], sum[2], inc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint4 *p = reinterpret_cast<const uint4 *>(hist + s * TG_BINS + t * 8);
        const uint4 lo = p[0], hi = p[1];
        b[s][0] = lo.x, b[s][1] = lo.y, b[s][2] = lo.z, b[s][3] = lo.w;
        b[s][4] = hi.x, b[s][5] = hi.y, b[s][6] = hi.z, b[s][7] = hi.w;
        sum[s] = ((b[s][0] + b[s][1]) + (b[s][2] + b[s][3])) + ((b[s][4] + b[s][5]) + (b[s][6] + b[s][7]));
        inc[s] = gs_wave_incl_scan_u32(sum[s]);
        if (lane == 63) s_wt[s][wv] = inc[s];
    }
    if (t < 4) s_res[t >> 1][t & 1] = 0u;
    __syncthreads();
    tg_pick out;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        uint32_t off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TG_BLOCK / 64; ++w) {
            const uint32_t v = s_wt[s][w];
            off += w < wv ? v : 0u;
            total += v;
        }
        out.total[s] = total;
        const uint32_t rank = MEDIAN ? (total ? (total - 1u) >> 1 : 0u) : (s == 0 ? rank_d : rank_c);
        const uint32_t excl = off + inc[s] - sum[s];
        if (rank >= excl && rank - excl < sum[s]) {  // (at most one thread: the bins partition the ranks)
            uint32_t r = rank - excl, bin = 0, left = 0;
            bool found = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (!found && r < b[s][j]) {
                    found = true;
                    bin = (uint32_t)(t * 8 + j);
                    left = r;
                }
                if (!found) r -= b[s][j];
            }
            s_res[s][0] = bin;
            s_res[s][1] = left;
        }
    }
    __syncthreads();
    out.bin[0] = s_res[0][0], out.rank[0] = s_res[0][1];
    out.bin[1] = s_res[1][0], out.rank[1] = s_res[1][1];
    return out;
}

// pass 2: a and c of one pixel (NaN outside the sets), and their level-0 digits into the workgroup's counters
template <bool RANGE>
__device__ __forceinline__ void track_gate_residual_pixel(float i0, float i1, float i2, float t0, float t1, float t2, float D,
                                                          float A, float z, float alpha_min, float &ra, float &rc,
                                                          uint32_t *s_h) {
    const float nan = __uint_as_float(0x7fc00000u);
    ra = rc = nan;
    if (!(A >= alpha_min)) return;  // (false for NaN)
    const float d0 = i0 - t0, d1 = i1 - t1, d2 = i2 - t2;
    const float c = (fabsf(d0) + fabsf(d1)) + fabsf(d2);
    if (c <= TG_FLT_MAX) rc = c;
    tg_count<0>(rc, 0u, s_h + TG_BINS);
    if (!RANGE) return;
    if (!map_measured(z)) return;
    float e;
    const float a = fabsf(map_expected_residual(D, A, z, e));
    if (a <= TG_FLT_MAX) ra = a;
    tg_count<0>(ra, 0u, s_h);
}

template <bool RANGE>
__global__ void __launch_bounds__(TG_BLOCK)
    track_gate_residual_kernel(const float *__restrict__ image, const float *__restrict__ depth, const float *__restrict__ alpha,
                               const float *__restrict__ target_image, const float *__restrict__ target_range, int64_t n,
                               int chunks, float alpha_min, float *__restrict__ resid_a, float *__restrict__ resid_c,
                               uint32_t *__restrict__ hist) {
    __shared__ uint32_t s_h[2 * TG_BINS];
    tg_zero_lds(s_h);
    __syncthreads();
    for (int it = 0; it < chunks; ++it) {
        const int64_t i0 = (((int64_t)blockIdx.x * chunks + it) * TG_BLOCK + threadIdx.x) * 4;
        if (i0 + 4 <= n) {
            const float4 d = *reinterpret_cast<const float4 *>(depth + i0), a = *reinterpret_cast<const float4 *>(alpha + i0);
            float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            if (RANGE) z = *reinterpret_cast<const float4 *>(target_range + i0);
            const float4 *pi = reinterpret_cast<const float4 *>(image + i0 * 3);
            const float4 *pt = reinterpret_cast<const float4 *>(target_image + i0 * 3);
            const float4 ia = pi[0], ib = pi[1], ic = pi[2], ta = pt[0], tb = pt[1], tc = pt[2];
            float4 ra, rc;
            track_gate_residual_pixel<RANGE>(ia.x, ia.y, ia.z, ta.x, ta.y, ta.z, d.x, a.x, z.x, alpha_min, ra.x, rc.x, s_h);
            track_gate_residual_pixel<RANGE>(ia.w, ib.x, ib.y, ta.w, tb.x, tb.y, d.y, a.y, z.y, alpha_min, ra.y, rc.y, s_h);
            track_gate_residual_pixel<RANGE>(ib.z, ib.w, ic.x, tb.z, tb.w, tc.x, d.z, a.z, z.z, alpha_min, ra.z, rc.z, s_h);
            track_gate_residual_pixel<RANGE>(ic.y, ic.z, ic.w, tc.y, tc.z, tc.w, d.w, a.w, z.w, alpha_min, ra.w, rc.w, s_h);
            *reinterpret_cast<float4 *>(resid_a + i0) = ra;
            *reinterpret_cast<float4 *>(resid_c + i0) = rc;
        } else {
            for (int64_t i = i0; i < n; ++i) {  // the up to three pixels an image whose size is no multiple of four ends with
                float ra, rc;
                track_gate_residual_pixel<RANGE>(image[i * 3], image[i * 3 + 1], image[i * 3 + 2], target_image[i * 3],
                                                 target_image[i * 3 + 1], target_image[i * 3 + 2], depth[i], alpha[i],
                                                 RANGE ? target_range[i] : 0.f, alpha_min, ra, rc, s_h);
                resid_a[i] = ra;
                resid_c[i] = rc;
            }
        }
    }
    __syncthreads();
    tg_flush_lds(s_h, hist);
}

// passes 3 and 4 (L = 1, 2): pick the bin of level L - 1, count level L's digit of the elements under the prefix so far
template <int L>
__global__ void __launch_bounds__(TG_BLOCK)
    track_gate_digit_kernel(const float *__restrict__ resid_a, const float *__restrict__ resid_c, int64_t n, int chunks,
                            uint32_t *__restrict__ hist, uint32_t *__restrict__ state) {
    __shared__ uint32_t s_h[2 * TG_BINS];
    tg_zero_lds(s_h);
    uint32_t pre_d, pre_c;
    const uint32_t *prev = hist + (L - 1) * 2 * TG_BINS;
    if (L == 1) {
        const tg_pick p = track_gate_select<true>(prev, 0u, 0u);
        pre_d = p.bin[0], pre_c = p.bin[1];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state[TG_BIN0_D] = p.bin[0], state[TG_RANK1_D] = p.rank[0];
            state[TG_BIN0_C] = p.bin[1], state[TG_RANK1_C] = p.rank[1];
            state[TG_N_D] = p.total[0], state[TG_N_C] = p.total[1];
        }
    } else {
        const tg_pick p = track_gate_select<false>(prev, state[TG_RANK1_D], state[TG_RANK1_C]);
        pre_d = (state[TG_BIN0_D] << 11) | p.bin[0], pre_c = (state[TG_BIN0_C] << 11) | p.bin[1];
        if (blockIdx.x == 0 && threadIdx.x == 0) {  // (words nobody reads in this launch)
            state[TG_BIN1_D] = p.bin[0], state[TG_RANK2_D] = p.rank[0];
            state[TG_BIN1_C] = p.bin[1], state[TG_RANK2_C] = p.rank[1];
        }
    }
    // (track_gate_select ended with a barrier: the counters are zero in every thread's view)
    for (int it = 0; it < chunks; ++it) {
        const int64_t i0 = (((int64_t)blockIdx.x * chunks + it) * TG_BLOCK + threadIdx.x) * 4;
        if (i0 + 4 <= n) {
            const float4 a = *reinterpret_cast<const float4 *>(resid_a + i0), c = *reinterpret_cast<const float4 *>(resid_c + i0);
            tg_count<L>(a.x, pre_d, s_h), tg_count<L>(a.y, pre_d, s_h), tg_count<L>(a.z, pre_d, s_h), tg_count<L>(a.w, pre_d, s_h);
            tg_count<L>(c.x, pre_c, s_h + TG_BINS), tg_count<L>(c.y, pre_c, s_h + TG_BINS);
            tg_count<L>(c.z, pre_c, s_h + TG_BINS), tg_count<L>(c.w, pre_c, s_h + TG_BINS);
        } else {
            for (int64_t i = i0; i < n; ++i) {
                tg_count<L>(resid_a[i], pre_d, s_h);
                tg_count<L>(resid_c[i], pre_c, s_h + TG_BINS);
            }
        }
    }
    __syncthreads();
    tg_flush_lds(s_h, hist + L * 2 * TG_BINS);
}

struct tg_sums {
    float colour, depth;
    uint32_t dcnt, ccnt;
};
struct tg_gate {
    float alpha_min, cs, ds, kd, kc, td, tc;
    int couple;
};

// pass 5, one pixel: track_loss_pixel with the two decisions taken from the stored residuals (ra, rc: NaN outside the sets)
template <bool RANGE>
__device__ __forceinline__ void track_gate_pixel(float i0, float i1, float i2, float t0, float t1, float t2, float D, float A,
                                                 float z, float ra, float rc, const tg_gate &G, float &g0, float &g1, float &g2,
                                                 float &gD, float &gA, tg_sums &acc) {
    g0 = g1 = g2 = gD = gA = 0.f;
    if (!(A >= G.alpha_min)) return;  // (false for NaN)
    bool depth_in = false, dropped = false;
    if (RANGE && map_measured(z)) {
        const bool in_set = ra <= TG_FLT_MAX;
        depth_in = !(G.kd > 0.f) || (in_set && ra <= G.td);
        dropped = G.couple && in_set && !depth_in;  // (depth_in is false only with the gate on)
    }
    if (!dropped && (!(G.kc > 0.f) || (rc <= TG_FLT_MAX && rc <= G.tc))) {
        const float d0 = i0 - t0, d1 = i1 - t1, d2 = i2 - t2;
        g0 = map_signed(d0, G.cs);
        g1 = map_signed(d1, G.cs);
        g2 = map_signed(d2, G.cs);
        acc.colour += (fabsf(d0) + fabsf(d1)) + fabsf(d2);
        ++acc.ccnt;
    }
    if (!depth_in) return;
    float e;
    const float r = map_expected_residual(D, A, z, e);
    ++acc.dcnt;
    const float sg = map_signed(r, G.ds);
    map_expected_grads(sg, e, A, gD, gA);
    acc.depth += fabsf(r);
}

template <bool RANGE>
__global__ void __launch_bounds__(TG_BLOCK)
    track_gate_loss_kernel(const float *__restrict__ image, const float *__restrict__ depth, const float *__restrict__ alpha,
                           const float *__restrict__ target_image, const float *__restrict__ target_range,
                           const float *__restrict__ resid_a, const float *__restrict__ resid_c, int64_t n, float alpha_min,
                           float cs, float ds, float kd, float kc, float floor_d, float floor_c, int couple,
                           const uint32_t *__restrict__ hist, uint32_t *__restrict__ state, float *__restrict__ grad_image,
                           float *__restrict__ grad_depth, float *__restrict__ grad_alpha, float4 *__restrict__ part) {
    __shared__ float s_col[TG_BLOCK / 64], s_dep[TG_BLOCK / 64];
    __shared__ uint32_t s_dc[TG_BLOCK / 64], s_cc[TG_BLOCK / 64];
    // the last level's pick completes both medians' bit patterns
    const tg_pick p = track_gate_select<false>(hist + 2 * 2 * TG_BINS, state[TG_RANK2_D], state[TG_RANK2_C]);
    const float m_d = __uint_as_float((state[TG_BIN0_D] << 21) | (state[TG_BIN1_D] << 10) | p.bin[0]);
    const float m_c = __uint_as_float((state[TG_BIN0_C] << 21) | (state[TG_BIN1_C] << 10) | p.bin[1]);
    tg_gate G;
    G.alpha_min = alpha_min, G.cs = cs, G.ds = ds, G.kd = kd, G.kc = kc, G.couple = couple;
    G.td = fmaxf(kd * m_d, floor_d);
    G.tc = fmaxf(kc * m_c, floor_c);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (for the finalize kernel; nobody reads them in this launch)
        state[TG_M_D] = __float_as_uint(m_d), state[TG_M_C] = __float_as_uint(m_c);
        state[TG_T_D] = __float_as_uint(G.td), state[TG_T_C] = __float_as_uint(G.tc);
    }
    const int64_t i0 = ((int64_t)blockIdx.x * TG_BLOCK + threadIdx.x) * 4;
    tg_sums acc = {0.f, 0.f, 0u, 0u};
    if (i0 + 4 <= n) {
        const float4 d = *reinterpret_cast<const float4 *>(depth + i0), a = *reinterpret_cast<const float4 *>(alpha + i0);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RANGE) z = *reinterpret_cast<const float4 *>(target_range + i0);
        const float4 ra = *reinterpret_cast<const float4 *>(resid_a + i0), rc = *reinterpret_cast<const float4 *>(resid_c + i0);
        const float4 *pi = reinterpret_cast<const float4 *>(image + i0 * 3);
        const float4 *pt = reinterpret_cast<const float4 *>(target_image + i0 * 3);
        const float4 ia = pi[0], ib = pi[1], ic = pi[2], ta = pt[0], tb = pt[1], tc = pt[2];
        float4 ga, gb, gc, gd, gal;  // (ga, gb, gc: the twelve colour gradients of the four pixels in memory order)
        track_gate_pixel<RANGE>(ia.x, ia.y, ia.z, ta.x, ta.y, ta.z, d.x, a.x, z.x, ra.x, rc.x, G, ga.x, ga.y, ga.z, gd.x, gal.x, acc);
        track_gate_pixel<RANGE>(ia.w, ib.x, ib.y, ta.w, tb.x, tb.y, d.y, a.y, z.y, ra.y, rc.y, G, ga.w, gb.x, gb.y, gd.y, gal.y, acc);
        track_gate_pixel<RANGE>(ib.z, ib.w, ic.x, tb.z, tb.w, tc.x, d.z, a.z, z.z, ra.z, rc.z, G, gb.z, gb.w, gc.x, gd.z, gal.z, acc);
        track_gate_pixel<RANGE>(ic.y, ic.z, ic.w, tc.y, tc.z, tc.w, d.w, a.w, z.w, ra.w, rc.w, G, gc.y, gc.z, gc.w, gd.w, gal.w, acc);
        float4 *po = reinterpret_cast<float4 *>(grad_image + i0 * 3);
        po[0] = ga;
        po[1] = gb;
        po[2] = gc;
        *reinterpret_cast<float4 *>(grad_depth + i0) = gd;
        *reinterpret_cast<float4 *>(grad_alpha + i0) = gal;
    } else {
        for (int64_t i = i0; i < n; ++i) {  // the up to three pixels an image whose size is no multiple of four ends with
            float g0, g1, g2, gd, ga;
            track_gate_pixel<RANGE>(image[i * 3], image[i * 3 + 1], image[i * 3 + 2], target_image[i * 3], target_image[i * 3 + 1],
                                    target_image[i * 3 + 2], depth[i], alpha[i], RANGE ? target_range[i] : 0.f, resid_a[i],
                                    resid_c[i], G, g0, g1, g2, gd, ga, acc);
            grad_image[i * 3] = g0;
            grad_image[i * 3 + 1] = g1;
            grad_image[i * 3 + 2] = g2;
            grad_depth[i] = gd;
            grad_alpha[i] = ga;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc.colour += __shfl_xor(acc.colour, o, 64);
        acc.depth += __shfl_xor(acc.depth, o, 64);
        acc.dcnt += __shfl_xor(acc.dcnt, o, 64);
        acc.ccnt += __shfl_xor(acc.ccnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_col[threadIdx.x >> 6] = acc.colour;
        s_dep[threadIdx.x >> 6] = acc.depth;
        s_dc[threadIdx.x >> 6] = acc.dcnt;
        s_cc[threadIdx.x >> 6] = acc.ccnt;
    }
    __syncthreads();
    if (threadIdx.x == 0)  // (a count is at most 1,024: exact as a float)
        part[blockIdx.x] = make_float4(((s_col[0] + s_col[1]) + s_col[2]) + s_col[3], ((s_dep[0] + s_dep[1]) + s_dep[2]) + s_dep[3],
                                       (float)(((s_dc[0] + s_dc[1]) + s_dc[2]) + s_dc[3]),
                                       (float)(((s_cc[0] + s_cc[1]) + s_cc[2]) + s_cc[3]));
}

// values_out = (loss, colour term, depth term, depth pixels that counted, colour pixels that counted, m_d, m_c, n_d): the
// sums as in track_loss_finalize_kernel (gs_common.h)
__global__ void __launch_bounds__(1024) track_gate_finalize_kernel(const float4 *__restrict__ part, int64_t nrows, float scale,
                                                                   float color_weight, float depth_weight,
                                                                   const uint32_t *__restrict__ state,
                                                                   float *__restrict__ values_out) {
    __shared__ double s_w[16][4];
    double c = 0.0, d = 0.0, k = 0.0, q = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += 1024) {
        const float4 v = part[r];
        c += (double)v.x;
        d += (double)v.y;
        k += (double)v.z;
        q += (double)v.w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o, 64);
        d += __shfl_xor(d, o, 64);
        k += __shfl_xor(k, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6][0] = c;
        s_w[threadIdx.x >> 6][1] = d;
        s_w[threadIdx.x >> 6][2] = k;
        s_w[threadIdx.x >> 6][3] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4];
        for (int j = 0; j < 4; ++j) {
            t[j] = s_w[0][j];
            for (int w = 1; w < 16; ++w) t[j] += s_w[w][j];
        }
        const double colour = (double)scale * (double)color_weight * t[0], dep = (double)scale * (double)depth_weight * t[1];
        values_out[0] = (float)(colour + dep);
        values_out[1] = (float)colour;
        values_out[2] = (float)dep;
        values_out[3] = (float)t[2];
        values_out[4] = (float)t[3];
        values_out[5] = __uint_as_float(state[TG_M_D]);
        values_out[6] = __uint_as_float(state[TG_M_C]);
        values_out[7] = (float)state[TG_N_D];  // (at most 2^24: exact)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// gs_track_gate_mask: the same sets, medians and thresholds, turned into the mapping inputs of a keyframe instead of a loss --
// a range map without the measurements the depth gate rejects and a 0 / 1 colour weight.  The memset, the residual pass and
// the two digit passes are the ones above; gate_mask_kernel takes the loss pass's place (it reads alpha, the range and the
// two residual maps: 16 B / pixel, writes 8) and gate_mask_finalize_kernel adds the workgroups' counts.
struct tg_counts {
    uint32_t measured, kept, wsum, wint;
};

// one pixel: the decisions of track_gate_pixel, -> the range and the weight the pixel keeps
template <bool RANGE>
__device__ __forceinline__ void gate_mask_pixel(float A, float z, float ra, float rc, bool interior, const tg_gate &G, float &zo,
                                                float &wo, tg_counts &acc) {
    const bool covered = A >= G.alpha_min;  // (false for NaN)
    const bool meas = RANGE && map_measured(z);
    bool removed = false, dropped = false;
    if (covered && meas) {
        const bool in_set = ra <= TG_FLT_MAX;
        const bool depth_in = !(G.kd > 0.f) || (in_set && ra <= G.td);
        removed = !depth_in;
        dropped = G.couple && in_set && !depth_in;
    }
    const bool colour_in = !dropped && (!(G.kc > 0.f) || (rc <= TG_FLT_MAX && rc <= G.tc));
    zo = (meas && !removed) ? z : 0.f;
    wo = (covered && !colour_in) ? 0.f : 1.f;
    acc.measured += meas ? 1u : 0u;
    acc.kept += (meas && !removed) ? 1u : 0u;
    acc.wsum += wo != 0.f ? 1u : 0u;
    acc.wint += (wo != 0.f && interior) ? 1u : 0u;
}

template <bool RANGE>
__global__ void __launch_bounds__(TG_BLOCK)
    gate_mask_kernel(const float *__restrict__ alpha, const float *__restrict__ target_range, const float *__restrict__ resid_a,
                     const float *__restrict__ resid_c, int64_t n, int32_t H, int32_t W, float alpha_min, float kd, float kc,
                     float floor_d, float floor_c, int couple, const uint32_t *__restrict__ hist, uint32_t *__restrict__ state,
                     float *__restrict__ range_out, float *__restrict__ weight_out, uint4 *__restrict__ part) {
    __shared__ uint32_t s_cnt[4][TG_BLOCK / 64];
    // the last level's pick completes both medians' bit patterns (as in track_gate_loss_kernel)
    const tg_pick p = track_gate_select<false>(hist + 2 * 2 * TG_BINS, state[TG_RANK2_D], state[TG_RANK2_C]);
    const float m_d = __uint_as_float((state[TG_BIN0_D] << 21) | (state[TG_BIN1_D] << 10) | p.bin[0]);
    const float m_c = __uint_as_float((state[TG_BIN0_C] << 21) | (state[TG_BIN1_C] << 10) | p.bin[1]);
    tg_gate G;
    G.alpha_min = alpha_min, G.cs = 0.f, G.ds = 0.f, G.kd = kd, G.kc = kc, G.couple = couple;
    G.td = fmaxf(kd * m_d, floor_d);
    G.tc = fmaxf(kc * m_c, floor_c);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (for the finalize kernel; nobody reads them in this launch)
        state[TG_M_D] = __float_as_uint(m_d), state[TG_M_C] = __float_as_uint(m_c);
        state[TG_T_D] = __float_as_uint(G.td), state[TG_T_C] = __float_as_uint(G.tc);
    }
    const int64_t i0 = ((int64_t)blockIdx.x * TG_BLOCK + threadIdx.x) * 4;
    tg_counts acc = {0u, 0u, 0u, 0u};
    // the SSIM interior: rows 5 .. H - 6, columns 5 .. W - 6 (n <= 2^24: the pixel index fits an int)
    auto interior = [&](int64_t i) {
        const int r = (int)i / W, c = (int)i - r * W;
        return r >= 5 && r < H - 5 && c >= 5 && c < W - 5;
    };
    if (i0 + 4 <= n) {
        const float4 a = *reinterpret_cast<const float4 *>(alpha + i0);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RANGE) z = *reinterpret_cast<const float4 *>(target_range + i0);
        const float4 ra = *reinterpret_cast<const float4 *>(resid_a + i0), rc = *reinterpret_cast<const float4 *>(resid_c + i0);
        float4 zo, wo;
        gate_mask_pixel<RANGE>(a.x, z.x, ra.x, rc.x, interior(i0), G, zo.x, wo.x, acc);
        gate_mask_pixel<RANGE>(a.y, z.y, ra.y, rc.y, interior(i0 + 1), G, zo.y, wo.y, acc);
        gate_mask_pixel<RANGE>(a.z, z.z, ra.z, rc.z, interior(i0 + 2), G, zo.z, wo.z, acc);
        gate_mask_pixel<RANGE>(a.w, z.w, ra.w, rc.w, interior(i0 + 3), G, zo.w, wo.w, acc);
        if (RANGE) *reinterpret_cast<float4 *>(range_out + i0) = zo;
        *reinterpret_cast<float4 *>(weight_out + i0) = wo;
    } else {
        for (int64_t i = i0; i < n; ++i) {  // the up to three pixels an image whose size is no multiple of four ends with
            float zo, wo;
            gate_mask_pixel<RANGE>(alpha[i], RANGE ? target_range[i] : 0.f, resid_a[i], resid_c[i], interior(i), G, zo, wo, acc);
            if (RANGE) range_out[i] = zo;
            weight_out[i] = wo;
        }
    }
    acc.measured = gs_wave_sum_u32(acc.measured);
    acc.kept = gs_wave_sum_u32(acc.kept);
    acc.wsum = gs_wave_sum_u32(acc.wsum);
    acc.wint = gs_wave_sum_u32(acc.wint);
    if ((threadIdx.x & 63) == 0) {
        s_cnt[0][threadIdx.x >> 6] = acc.measured;
        s_cnt[1][threadIdx.x >> 6] = acc.kept;
        s_cnt[2][threadIdx.x >> 6] = acc.wsum;
        s_cnt[3][threadIdx.x >> 6] = acc.wint;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        part[blockIdx.x] = make_uint4(((s_cnt[0][0] + s_cnt[0][1]) + s_cnt[0][2]) + s_cnt[0][3],
                                      ((s_cnt[1][0] + s_cnt[1][1]) + s_cnt[1][2]) + s_cnt[1][3],
                                      ((s_cnt[2][0] + s_cnt[2][1]) + s_cnt[2][2]) + s_cnt[2][3],
                                      ((s_cnt[3][0] + s_cnt[3][1]) + s_cnt[3][2]) + s_cnt[3][3]);
}

// values_out = (measured pixels, range pixels kept, range pixels removed, sum of the weights, the same over the SSIM interior,
// m_d, m_c, n_d): integer sums (at most H W <= 2^24: exact as floats) of the workgroups' rows, in the fixed order of gs_common.h
__global__ void __launch_bounds__(1024) gate_mask_finalize_kernel(const uint4 *__restrict__ part, int64_t nrows,
                                                                  const uint32_t *__restrict__ state,
                                                                  float *__restrict__ values_out) {
    __shared__ uint32_t s_w[16][4];
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (int64_t r = threadIdx.x; r < nrows; r += 1024) {
        const uint4 v = part[r];
        c[0] += v.x, c[1] += v.y, c[2] += v.z, c[3] += v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = gs_wave_sum_u32(c[j]);
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6][j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t[4];
        for (int j = 0; j < 4; ++j) {
            t[j] = s_w[0][j];
            for (int w = 1; w < 16; ++w) t[j] += s_w[w][j];
        }
        values_out[0] = (float)t[0];
        values_out[1] = (float)t[1];
        values_out[2] = (float)(t[0] - t[1]);
        values_out[3] = (float)t[2];
        values_out[4] = (float)t[3];
        values_out[5] = __uint_as_float(state[TG_M_D]);
        values_out[6] = __uint_as_float(state[TG_M_C]);
        values_out[7] = (float)state[TG_N_D];  // (at most 2^24: exact)
    }
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (a NULL pointer overlaps nothing)
inline bool tg_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" size_t gs_loss_track_gated_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return tg_workspace((int64_t)H * W).total;
}

extern "C" int gs_loss_track_gated(const float *image, const float *depth, const float *alpha, const float *target_image,
                                   const float *target_range, int32_t H, int32_t W, float alpha_min, float color_weight,
                                   float depth_weight, float depth_gate_k, float color_gate_k, float depth_gate_floor,
                                   float color_gate_floor, int32_t couple, float scale, float *grad_image, float *grad_depth,
                                   float *grad_alpha, float *values_out, float *resid_depth, float *resid_color,
                                   void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    const int64_t n = (int64_t)H * W;
    GS_CHECK_ARG(n <= TG_MAX_PIXELS, "image size beyond 2^24 pixels (the counts are returned as floats and must be exact)");
    GS_CHECK_ARG(image && depth && alpha && target_image && grad_image && grad_depth && grad_alpha,
                 "null pointer (only target_range, values_out, resid_depth and resid_color may be NULL)");
    GS_CHECK_ARG(alpha_min > 0.f, "alpha_min must be positive (the expected depth divides by alpha)");
    GS_CHECK_ARG(color_weight >= 0.f && depth_weight >= 0.f, "color_weight and depth_weight must not be negative or NaN");
    GS_CHECK_ARG(!std::isnan(depth_gate_k) && !std::isnan(color_gate_k), "depth_gate_k and color_gate_k must not be NaN");
    GS_CHECK_ARG(depth_gate_floor >= 0.f && color_gate_floor >= 0.f, "the gate floors must not be negative or NaN");
    GS_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    {  // the kernels walk the maps float4 by float4
        const void *al[] = {image, depth, alpha, target_image, target_range, grad_image, grad_depth, grad_alpha, resid_depth,
                            resid_color};
        for (const void *q : al) GS_CHECK_ARG(((uintptr_t)q & 15) == 0, "the maps must be 16-byte aligned");
    }
    GS_CHECK_ARG(((uintptr_t)values_out & 3) == 0, "values_out must be 4-byte aligned");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= gs_loss_track_gated_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const tg_layout L = tg_workspace(n);
    char *ws = (char *)workspace;
    float4 *part = (float4 *)(ws + L.part);
    uint32_t *hist = (uint32_t *)(ws + L.hist), *state = (uint32_t *)(ws + L.state);
    float *ra = resid_depth ? resid_depth : (float *)(ws + L.resid_a);
    float *rc = resid_color ? resid_color : (float *)(ws + L.resid_c);
    const float cs = scale * color_weight, ds = scale * depth_weight;  // (one rounding each: -ffp-contract=off)
    const int64_t nchunks = tg_blocks(n);  // (at most 2^14)
    const unsigned blocks = (unsigned)nchunks;
    int rchunks = (int)gs_div_up(nchunks, TG_RESIDUAL_BLOCKS);
    if (rchunks > TG_RESIDUAL_MAX_CHUNKS) rchunks = TG_RESIDUAL_MAX_CHUNKS;
    const int dchunks = (int)gs_div_up(nchunks, TG_DIGIT_BLOCKS);
    const unsigned rblocks = (unsigned)gs_div_up(nchunks, rchunks), dblocks = (unsigned)gs_div_up(nchunks, dchunks);
    GS_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * TG_LEVELS * 2 * TG_BINS, s));
    if (target_range)
        hipLaunchKernelGGL(track_gate_residual_kernel<true>, dim3(rblocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, n, rchunks, alpha_min, ra, rc, hist);
    else
        hipLaunchKernelGGL(track_gate_residual_kernel<false>, dim3(rblocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, n, rchunks, alpha_min, ra, rc, hist);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gate_digit_kernel<1>, dim3(dblocks), dim3(TG_BLOCK), 0, s, (const float *)ra, (const float *)rc, n, dchunks,
                       hist, state);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gate_digit_kernel<2>, dim3(dblocks), dim3(TG_BLOCK), 0, s, (const float *)ra, (const float *)rc, n, dchunks,
                       hist, state);
    GS_CHECK_LAUNCH();
    if (target_range)
        hipLaunchKernelGGL(track_gate_loss_kernel<true>, dim3(blocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, (const float *)ra, (const float *)rc, n, alpha_min, cs, ds, depth_gate_k, color_gate_k,
                           depth_gate_floor, color_gate_floor, couple != 0, (const uint32_t *)hist, state, grad_image, grad_depth,
                           grad_alpha, part);
    else
        hipLaunchKernelGGL(track_gate_loss_kernel<false>, dim3(blocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, (const float *)ra, (const float *)rc, n, alpha_min, cs, ds, depth_gate_k, color_gate_k,
                           depth_gate_floor, color_gate_floor, couple != 0, (const uint32_t *)hist, state, grad_image, grad_depth,
                           grad_alpha, part);
    GS_CHECK_LAUNCH();
    if (values_out) {
        hipLaunchKernelGGL(track_gate_finalize_kernel, dim3(1), dim3(1024), 0, s, (const float4 *)part, (int64_t)blocks, scale,
                           color_weight, depth_weight, (const uint32_t *)state, values_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" size_t gs_track_gate_mask_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return tg_workspace((int64_t)H * W).total;
}

extern "C" int gs_track_gate_mask(const float *image, const float *depth, const float *alpha, const float *target_image,
                                  const float *target_range, int32_t H, int32_t W, float alpha_min, float depth_gate_k,
                                  float color_gate_k, float depth_gate_floor, float color_gate_floor, int32_t couple,
                                  float *range_out, float *weight_out, float *values_out, float *resid_depth,
                                  float *resid_color, void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    const int64_t n = (int64_t)H * W;
    GS_CHECK_ARG(n <= TG_MAX_PIXELS, "image size beyond 2^24 pixels (the counts are returned as floats and must be exact)");
    GS_CHECK_ARG(image && depth && alpha && target_image && weight_out,
                 "null pointer (only target_range with range_out, values_out, resid_depth and resid_color may be NULL)");
    GS_CHECK_ARG((target_range != nullptr) == (range_out != nullptr),
                 "target_range and range_out must both be given or both be NULL");
    GS_CHECK_ARG(alpha_min > 0.f, "alpha_min must be positive (the expected depth divides by alpha)");
    GS_CHECK_ARG(!std::isnan(depth_gate_k) && !std::isnan(color_gate_k), "depth_gate_k and color_gate_k must not be NaN");
    GS_CHECK_ARG(depth_gate_floor >= 0.f && color_gate_floor >= 0.f, "the gate floors must not be negative or NaN");
    {  // the kernels walk the maps float4 by float4
        const void *al[] = {image, depth, alpha, target_image, target_range, range_out, weight_out, resid_depth, resid_color};
        for (const void *q : al) GS_CHECK_ARG(((uintptr_t)q & 15) == 0, "the maps must be 16-byte aligned");
    }
    GS_CHECK_ARG(((uintptr_t)values_out & 3) == 0, "values_out must be 4-byte aligned");
    {  // an output that shares a byte with an input (or with another output) would be read after it was written
        const size_t b1 = sizeof(float) * (size_t)n, b3 = 3 * b1;
        const struct {
            const void *p;
            size_t bytes;
        } in[] = {{image, b3}, {depth, b1}, {alpha, b1}, {target_image, b3}, {target_range, b1}},
          out[] = {{range_out, b1}, {weight_out, b1}, {values_out, 8 * sizeof(float)}, {resid_depth, b1}, {resid_color, b1}};
        for (const auto &o : out)
            for (const auto &i : in) GS_CHECK_ARG(!tg_overlap(o.p, o.bytes, i.p, i.bytes), "an output overlaps an input");
        for (size_t u = 0; u < 5; ++u)
            for (size_t v = u + 1; v < 5; ++v)
                GS_CHECK_ARG(!tg_overlap(out[u].p, out[u].bytes, out[v].p, out[v].bytes), "two outputs overlap");
    }
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= gs_track_gate_mask_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const tg_layout L = tg_workspace(n);
    char *ws = (char *)workspace;
    uint4 *part = (uint4 *)(ws + L.part);
    uint32_t *hist = (uint32_t *)(ws + L.hist), *state = (uint32_t *)(ws + L.state);
    float *ra = resid_depth ? resid_depth : (float *)(ws + L.resid_a);
    float *rc = resid_color ? resid_color : (float *)(ws + L.resid_c);
    const int64_t nchunks = tg_blocks(n);  // (at most 2^14)
    const unsigned blocks = (unsigned)nchunks;
    int rchunks = (int)gs_div_up(nchunks, TG_RESIDUAL_BLOCKS);
    if (rchunks > TG_RESIDUAL_MAX_CHUNKS) rchunks = TG_RESIDUAL_MAX_CHUNKS;
    const int dchunks = (int)gs_div_up(nchunks, TG_DIGIT_BLOCKS);
    const unsigned rblocks = (unsigned)gs_div_up(nchunks, rchunks), dblocks = (unsigned)gs_div_up(nchunks, dchunks);
    GS_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * TG_LEVELS * 2 * TG_BINS, s));
    if (target_range)
        hipLaunchKernelGGL(track_gate_residual_kernel<true>, dim3(rblocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, n, rchunks, alpha_min, ra, rc, hist);
    else
        hipLaunchKernelGGL(track_gate_residual_kernel<false>, dim3(rblocks), dim3(TG_BLOCK), 0, s, image, depth, alpha, target_image,
                           target_range, n, rchunks, alpha_min, ra, rc, hist);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gate_digit_kernel<1>, dim3(dblocks), dim3(TG_BLOCK), 0, s, (const float *)ra, (const float *)rc, n, dchunks,
                       hist, state);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gate_digit_kernel<2>, dim3(dblocks), dim3(TG_BLOCK), 0, s, (const float *)ra, (const float *)rc, n, dchunks,
                       hist, state);
    GS_CHECK_LAUNCH();
    if (target_range)
        hipLaunchKernelGGL(gate_mask_kernel<true>, dim3(blocks), dim3(TG_BLOCK), 0, s, alpha, target_range, (const float *)ra,
                           (const float *)rc, n, H, W, alpha_min, depth_gate_k, color_gate_k, depth_gate_floor, color_gate_floor,
                           couple != 0, (const uint32_t *)hist, state, range_out, weight_out, part);
    else
        hipLaunchKernelGGL(gate_mask_kernel<false>, dim3(blocks), dim3(TG_BLOCK), 0, s, alpha, target_range, (const float *)ra,
                           (const float *)rc, n, H, W, alpha_min, depth_gate_k, color_gate_k, depth_gate_floor, color_gate_floor,
                           couple != 0, (const uint32_t *)hist, state, range_out, weight_out, part);
    GS_CHECK_LAUNCH();
    if (values_out) {
        hipLaunchKernelGGL(gate_mask_finalize_kernel, dim3(1), dim3(1024), 0, s, (const uint4 *)part, (int64_t)blocks,
                           (const uint32_t *)state, values_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
