// map_edit.hip -- editing the Gaussian set of a running fit: remove rows by one per-row decision and move whatever shares the
// row index with them (gs_prune_classify / gs_prune_apply, include/gs_abi.h).
//
// A mapping loop only appends Gaussians (seed.hip); the ones training drove to zero opacity, or blew up, stay and are
// projected, binned and stepped by Adam for the rest of the run.  Removing them is a stable compaction of every array that is
// addressed by the Gaussian's row: the five parameter arrays, the optimizer's ten moment arrays, the densification statistic
// -- sixteen boolean-mask gathers in torch.  Here, three launches in the manner of seed.hip:
//   P1 prune_classify_kernel : a thread per row decides; the wave's ballot (8 bytes per 64 rows) and the workgroup's kept
//                              count go to the workspace;
//   P2 prune_scan_kernel     : exclusive scan of the workgroups' counts, totals -> counts_dev = (kept, removed);
//   P3 prune_apply_kernel    : a workgroup per 256 source rows.  Its kept rows are consecutive destination rows of EVERY
//                              array, so it builds one 256-entry LDS table kept-rank -> source row from the ballots and then
//                              walks, array by array, the floats of its destination span with consecutive lanes on
//                              consecutive floats: whole lines out, runs of whole rows in.  A row's width only sets how many
//                              floats the span has -- rows of 1, 3, 4, 27 and 48 floats take the same loop.
// The decision is the delete rule of densify.hip's classify with both thresholds as arguments, restated here (no device code
// is shared: densify.hip stays as it is):
//   keep  <=>  opa[i] > opa_logit_min  and  norm < scale_max,   norm = sqrtf(a a + b b + c c), (a, b, c) = |s| or expf(s)
// in fp32 with one rounding per operation (the file is compiled with -ffp-contract=off); a NaN on either side is not kept.
// With scale_max = +inf the second test passes every finite norm (an infinite or NaN norm is still not kept).
// The rank of a kept row is the number of kept rows before it: the output is a pure function of the inputs, no slot is claimed
// with an atomic, two runs give the same bytes whatever the workspace held.  Nothing is written when dst_offset + kept exceeds
// `capacity` (counts_dev still holds the need: the convention of gs_densify_apply and gs_seed_apply).
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int PRUNE_BLOCK = 256, PRUNE_WAVES = PRUNE_BLOCK / 64;

__device__ __forceinline__ float prune_act_norm(const float *s, int scale_act) {
    const float a = scale_act == 0 ? fabsf(s[0]) : expf(s[0]);
    const float b = scale_act == 0 ? fabsf(s[1]) : expf(s[1]);
    const float c = scale_act == 0 ? fabsf(s[2]) : expf(s[2]);
    return sqrtf(a * a + b * b + c * c);
}

__global__ void __launch_bounds__(PRUNE_BLOCK) prune_classify_kernel(const float *__restrict__ scale,
                                                                    const float *__restrict__ opa, int64_t n,
                                                                    float opa_logit_min, float scale_max, int scale_act,
                                                                    unsigned long long *__restrict__ masks,
                                                                    uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t s_keep[PRUNE_WAVES];
    const int64_t i = (int64_t)blockIdx.x * PRUNE_BLOCK + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const float s[3] = {scale[i * 3], scale[i * 3 + 1], scale[i * 3 + 2]};
        const float norm = prune_act_norm(s, scale_act);
        keep = opa[i] > opa_logit_min && norm < scale_max;  // (both false for NaN)
    }
    const unsigned long long m = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * PRUNE_WAVES + wave] = m;
        s_keep[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
}

// prune_classify_kernel's decision with the contribution rule joined to it (gs_prune_classify_contrib): a kernel of its own
// beside it, the same ballots and counts out.  rows[i] = (weight_sum, weight_max, pixels, views) of gs_frame_contrib; a NaN
// weight_max fails its comparison: not kept.
__global__ void __launch_bounds__(PRUNE_BLOCK) prune_classify_contrib_kernel(
    const float *__restrict__ scale, const float *__restrict__ opa, const uint4 *__restrict__ rows, int64_t n,
    float opa_logit_min, float scale_max, int scale_act, float weight_max_min, uint32_t pixels_min, uint32_t views_min,
    unsigned long long *__restrict__ masks, uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t s_keep[PRUNE_WAVES];
    const int64_t i = (int64_t)blockIdx.x * PRUNE_BLOCK + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const float s[3] = {scale[i * 3], scale[i * 3 + 1], scale[i * 3 + 2]};
        const float norm = prune_act_norm(s, scale_act);
        const uint4 r = rows[i];
        keep = opa[i] > opa_logit_min && norm < scale_max && __uint_as_float(r.y) >= weight_max_min && r.z >= pixels_min &&
               r.w >= views_min;
    }
    const unsigned long long m = __ballot(keep);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * PRUNE_WAVES + wave] = m;
        s_keep[wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
}

// one workgroup, trips of 1,024 counts: block_counts[i] <- exclusive scan; counts = (kept, n - kept)
__global__ void __launch_bounds__(1024) prune_scan_kernel(uint32_t *__restrict__ block_counts, int nblk, int64_t n,
                                                          long long *__restrict__ counts) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < nblk ? block_counts[i] : 0;
        const uint32_t incl = gs_wave_incl_scan_u32(v);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t off = 0, t = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? s_wave[w] : 0;
            t += s_wave[w];
        }
        if (i < nblk) block_counts[i] = s_carry + off + incl - v;
        const uint32_t next = s_carry + t;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = next;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = s_carry;
        counts[1] = n - (long long)s_carry;
    }
}

// the arrays of one call, by value in the kernel arguments; `magic` = floor(2^32 / width) + 1: e / width for e * width < 2^32
struct PruneTable {
    int32_t n;
    uint32_t width[GS_PRUNE_MAX_ARRAYS], magic[GS_PRUNE_MAX_ARRAYS];
    const float *src[GS_PRUNE_MAX_ARRAYS];
    float *dst[GS_PRUNE_MAX_ARRAYS];
};
constexpr uint32_t PRUNE_MAGIC_WIDTHS = 4096;  // 256 rows x width^2 < 2^32 below this: the multiply-high quotient is exact

__global__ void __launch_bounds__(PRUNE_BLOCK) prune_apply_kernel(PruneTable T, int64_t n, int64_t dst_offset,
                                                                 int64_t capacity,
                                                                 const unsigned long long *__restrict__ masks,
                                                                 const uint32_t *__restrict__ block_offsets,
                                                                 const long long *__restrict__ counts) {
    __shared__ uint32_t s_src[PRUNE_BLOCK];  // kept rank within the workgroup -> row within the workgroup
    const int64_t need = counts[0];
    if (need < 0 || dst_offset + need > capacity) return;  // (the whole grid alike; the host reads the same count)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * PRUNE_BLOCK;
    // the ballots, cut to the rows that exist: whatever the workspace holds, every table entry below `cnt` is written and
    // names a row < n
    uint32_t before = 0, total = 0;
    unsigned long long mine = 0;
#pragma unroll
    for (int w = 0; w < PRUNE_WAVES; ++w) {
        const int64_t left = n - (row0 + w * 64);
        const unsigned long long valid = left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
        const unsigned long long m = masks[(size_t)blockIdx.x * PRUNE_WAVES + w] & valid;
        const uint32_t c = (uint32_t)__popcll(m);
        before += w < wave ? c : 0;
        total += c;
        mine = w == wave ? m : mine;
    }
    if ((mine >> lane) & 1ull) s_src[before + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull))] = threadIdx.x;
    __syncthreads();
    // (base + cnt <= need always holds for the workspace and counts of ONE classify call; a mismatched pair stays in bounds)
    const int64_t base = block_offsets[blockIdx.x];
    const int64_t room = need - base;
    const uint32_t cnt = room <= 0 ? 0u : (uint32_t)(room < (int64_t)total ? room : (int64_t)total);
    if (cnt == 0) return;
    for (int k = 0; k < T.n; ++k) {
        const uint32_t w = T.width[k], magic = T.magic[k];
        const float *__restrict__ src = T.src[k] + row0 * w;
        float *__restrict__ dst = T.dst[k] + (dst_offset + base) * w;
        if (w < PRUNE_MAGIC_WIDTHS) {
            const uint32_t span = cnt * w;
            // four loads in flight per lane before the first store: the walk is latency bound otherwise
            for (uint32_t e0 = threadIdx.x; e0 < span; e0 += 4 * PRUNE_BLOCK) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t e = e0 + j * PRUNE_BLOCK;
                    if (e < span) {
                        const uint32_t r = w == 1 ? e : __umulhi(e, magic);
                        v[j] = src[(size_t)s_src[r] * w + (e - r * w)];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t e = e0 + j * PRUNE_BLOCK;
                    if (e < span) dst[e] = v[j];
                }
            }
        } else {  // rows of 16 KiB and more: the same walk with 64-bit indices and a division
            const uint64_t span = (uint64_t)cnt * w;
            for (uint64_t e = threadIdx.x; e < span; e += PRUNE_BLOCK) {
                const uint64_t r = e / w;
                dst[e] = src[(size_t)s_src[r] * w + (e - r * w)];
            }
        }
    }
}

struct PruneWs {
    unsigned long long *masks;
    uint32_t *block_counts;
    size_t bytes;
};
PruneWs prune_carve(void *base, int64_t n) {
    PruneWs w;
    const int64_t nblk = gs_div_up(n > 0 ? n : 1, PRUNE_BLOCK);
    const size_t a = gs_align_up(sizeof(unsigned long long) * PRUNE_WAVES * (size_t)nblk, 256);
    w.masks = (unsigned long long *)base;
    w.block_counts = base ? (uint32_t *)((char *)base + a) : nullptr;
    w.bytes = a + gs_align_up(sizeof(uint32_t) * (size_t)nblk, 256);
    return w;
}

}  // namespace

extern "C" size_t gs_prune_workspace_bytes(int64_t N) { return N < 0 ? 0 : prune_carve(nullptr, N).bytes; }

extern "C" int gs_prune_classify(const float *scale, const float *opa, int64_t N, const gs_prune_opts *opts,
                                 int64_t *counts_dev, void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(opts != nullptr, "opts is null");
    GS_CHECK_ARG(std::isfinite(opts->opa_logit_min), "opa_logit_min must be finite");
    GS_CHECK_ARG(!std::isnan(opts->scale_max), "scale_max must not be NaN (+inf switches the test off)");
    GS_CHECK_ARG(opts->scale_activation == 0 || opts->scale_activation == 1, "scale_activation must be 0 (abs) or 1 (exp)");
    GS_CHECK_ARG(N >= 0 && N < (1ll << 31), "N out of range");
    GS_CHECK_ARG(counts_dev != nullptr, "counts_dev is null");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_prune_workspace_bytes(N),
                 "workspace null, misaligned or too small");
    GS_CHECK_ARG(N == 0 || (scale && opa), "scale or opa is null");
    hipStream_t s = (hipStream_t)stream;
    const PruneWs w = prune_carve(workspace, N);
    const int nblk = (int)gs_div_up(N, PRUNE_BLOCK);
    if (nblk > 0) {
        hipLaunchKernelGGL(prune_classify_kernel, dim3(nblk), dim3(PRUNE_BLOCK), 0, s, scale, opa, N, opts->opa_logit_min,
                           opts->scale_max, opts->scale_activation, w.masks, w.block_counts);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(1024), 0, s, w.block_counts, nblk, N, (long long *)counts_dev);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_prune_classify_contrib(const float *scale, const float *opa, const gs_contrib_row *rows, int64_t N,
                                         const gs_prune_opts *opts, const gs_prune_contrib_opts *copts, int64_t *counts_dev,
                                         void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(opts != nullptr, "opts is null");
    GS_CHECK_ARG(copts != nullptr, "copts is null");
    GS_CHECK_ARG(std::isfinite(opts->opa_logit_min), "opa_logit_min must be finite");
    GS_CHECK_ARG(!std::isnan(opts->scale_max), "scale_max must not be NaN (+inf switches the test off)");
    GS_CHECK_ARG(opts->scale_activation == 0 || opts->scale_activation == 1, "scale_activation must be 0 (abs) or 1 (exp)");
    GS_CHECK_ARG(copts->weight_max_min >= 0.f, "weight_max_min must not be NaN or negative");
    GS_CHECK_ARG(N >= 0 && N < (1ll << 31), "N out of range");
    GS_CHECK_ARG(counts_dev != nullptr, "counts_dev is null");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_prune_workspace_bytes(N),
                 "workspace null, misaligned or too small");
    GS_CHECK_ARG(N == 0 || (scale && opa), "scale or opa is null");
    GS_CHECK_ARG(N == 0 || rows != nullptr, "rows is null");
    GS_CHECK_ARG(((uintptr_t)rows & 15) == 0, "rows must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const PruneWs w = prune_carve(workspace, N);
    const int nblk = (int)gs_div_up(N, PRUNE_BLOCK);
    if (nblk > 0) {
        hipLaunchKernelGGL(prune_classify_contrib_kernel, dim3(nblk), dim3(PRUNE_BLOCK), 0, s, scale, opa,
                           reinterpret_cast<const uint4 *>(rows), N, opts->opa_logit_min, opts->scale_max,
                           opts->scale_activation, copts->weight_max_min, copts->pixels_min, copts->views_min, w.masks,
                           w.block_counts);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(1024), 0, s, w.block_counts, nblk, N, (long long *)counts_dev);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_prune_apply(const gs_prune_arrays *arrays, int64_t N, int64_t dst_offset, int64_t capacity,
                              const int64_t *counts_dev, const void *workspace, size_t workspace_bytes,
                              gs_stream_t stream) {
    GS_CHECK_ARG(arrays != nullptr, "arrays is null");
    GS_CHECK_ARG(arrays->n >= 1 && arrays->n <= GS_PRUNE_MAX_ARRAYS, "the number of arrays must lie in 1 .. 16");
    GS_CHECK_ARG(N >= 0 && N < (1ll << 31), "N out of range");
    GS_CHECK_ARG(dst_offset >= 0 && capacity >= 0, "dst_offset and capacity must not be negative");
    PruneTable T;
    T.n = arrays->n;
    for (int k = 0; k < GS_PRUNE_MAX_ARRAYS; ++k) {
        T.width[k] = T.magic[k] = 0;
        T.src[k] = nullptr;
        T.dst[k] = nullptr;
    }
    for (int k = 0; k < arrays->n; ++k) {
        GS_CHECK_ARG(arrays->width[k] >= 1, "a row width must be >= 1");
        // (an array of no rows has no address: src may be null with N = 0, dst with capacity = 0)
        GS_CHECK_ARG((N == 0 || arrays->src[k] != nullptr) && (capacity == 0 || arrays->dst[k] != nullptr),
                     "a src or dst pointer is null");
        T.width[k] = (uint32_t)arrays->width[k];
        T.magic[k] = T.width[k] > 1 ? (uint32_t)((1ull << 32) / T.width[k] + 1ull) : 0u;
        T.src[k] = arrays->src[k];
        T.dst[k] = arrays->dst[k];
    }
    for (int k = 0; k < arrays->n; ++k)
        for (int j = 0; j < arrays->n; ++j)
            GS_CHECK_ARG(arrays->dst[k] == nullptr || (const float *)arrays->dst[k] != arrays->src[j],
                         "a dst array is a src array (the move is not in place)");
    GS_CHECK_ARG(counts_dev != nullptr, "counts_dev is null");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_prune_workspace_bytes(N),
                 "workspace null, misaligned or too small");
    if (N == 0 || capacity <= dst_offset) return 0;  // no row can be moved
    const PruneWs w = prune_carve(const_cast<void *>(workspace), N);
    hipLaunchKernelGGL(prune_apply_kernel, dim3((unsigned)gs_div_up(N, PRUNE_BLOCK)), dim3(PRUNE_BLOCK), 0,
                       (hipStream_t)stream, T, N, dst_offset, capacity, w.masks, w.block_counts,
                       (const long long *)counts_dev);
    GS_CHECK_LAUNCH();
    return 0;
}
