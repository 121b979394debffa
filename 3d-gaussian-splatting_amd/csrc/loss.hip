// loss.hip -- the reference trainer's image loss and its gradient, fused.
//
// train.py:99-107:  loss = (1 - w) mean|x - y| + w (1 - SSIM(x, y)),  w = --ssim_weight (0.1),
// SSIM = torchmetrics.StructuralSimilarityIndexMeasure(data_range=1.0) (train.py:71; unpinned third-party
// dependency, absent here; algorithm restated from its published source, functional/image/ssim.py):
// 11x11 Gaussian window (sigma 1.5, separable, normalised), k1 = 0.01, k2 = 0.03; inputs are reflect-
// padded by 5, filtered with a VALID convolution and the result cropped by 5 again -- i.e. the SSIM map
// is evaluated exactly on the interior pixels whose window lies inside the image, and averaged over
// them and the 3 channels.  Per pixel, with mu = g*x, nu = g*y, Exx = g*x^2, Eyy = g*y^2, Exy = g*xy:
//   A1 = 2 mu nu + c1, A2 = 2 (Exy - mu nu) + c2, B1 = mu^2 + nu^2 + c1,
//   B2 = max(Exx - mu^2, 0) + max(Eyy - nu^2, 0) + c2,   S = A1 A2 / (B1 B2).
// torch autograd would run ~40 elementwise/conv kernels over 5 padded copies of the image for this.  With
//   D_mu = dS/dmu, D_xx = dS/dExx, D_xy = dS/dExy  (zero outside the interior),
//   dL/dx(q) = a sign(x - y) - b [ (g*D_mu)(q) + 2 x(q) (g*D_xx)(q) + y(q) (g*D_xy)(q) ],
//   a = (1 - w) / (3 H W), b = w / (3 (H - 10)(W - 10))  (g is symmetric)
// the whole thing is FOUR separable filter stages with a pointwise step in the middle, and it runs as ONE streaming
// kernel (loss_fused_kernel below; rounds 1 - 3 used two tiled passes with the nine adjoint planes in HBM between
// them, 143 us at 1080p) plus a one-block reduction.
// Images are [H, W, 3] fp32, the layout the rasterizer writes.
// gs_loss_l1_ssim_weighted is the same kernel with a per-pixel weight map (loss_weighted_kernel: the body is shared through
// loss_fused_body.inc) and the weighted L1-only kernel beside l1_only_kernel.
#include <type_traits>

#include "gs_common.h"

namespace {

constexpr int R = 5, K = 11;   // window radius / size
struct Window {
    float g[K];
};

struct LossGeom {
    int32_t H, W;
    float c1, c2, a, b;
};

template <int WAVES = 4>
__device__ __forceinline__ float block_sum(float v, float *s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) tot += s_red[w];
    return tot;
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused kernel.  The image is a matrix of H rows x F = 3 W floats (channels interleaved), so a horizontal tap of
// one channel is a stride-3 tap of the flat row and every load / store of a wave is contiguous.  A workgroup of FT
// threads owns a vertical strip of SH gradient rows: thread t <-> flat column c0 - 15 + t.  It walks DOWN the strip one
// image row per step and keeps everything vertical in registers:
//   row of x, y (FT + 30 columns) -> LDS
//   H1  h[5]   = horizontal filter of (x, y, xx, yy, xy) at the row                              all FT columns
//   V1  ring of 11 x 5 partial vertical sums; the one that is complete after row i is the moment vector of row i - 5
//   P   moments -> S (summed over the strip's own rows) and the three adjoints, zero outside the interior -> LDS row
//   H2  g[3]   = horizontal filter of the adjoint row                                      FT - 30 output columns
//   V2  ring of 11 x 3 partial sums; complete after row i: gradient row i - 10 (+ the L1 term), stored
// The loop is unrolled over the 11 phases of the rings, so every ring slot is a fixed register (133 VGPRs, no scratch).
// Costs against the two-pass version: the strip's first 20 rows and 30 of its FT columns are recomputed halo (SH = 52:
// 1.37 x on H1 / V1, 1.19 x on H2 / V2; FT = 512: 1.06 x), nothing else is -- no adjoint planes (75 MB written,
// ~165 MB read back), no second read of the image beyond the two values of the output pixel, 22 + 33 LDS reads per
// column and row.  Measured at 1080p (profiles/r03_ab_*): 0.146 -> 0.096 ms per loss evaluation; the kernel issues
// 35.3 M VALU wave instructions (255 per column-row step: 77 H1 + 55 V1 + ~30 P + 33 H2 + 33 V2 + ~25 addressing and
// masks) = 57 us of issue time on 1024 SIMDs, and runs 91 - 95 us: 12 x 21 = 252 workgroups, one per CU with two
// waves per SIMD.  Measured alternatives (same box): FT = 256 with two workgroups per CU 0.100 ms, FT = 256 / SH = 38
// (three per CU, 23 % more halo work) 0.098, FT = 768 0.102, FT = 1024 0.116 - 0.150, the three products staged in LDS
// next to x, y (5 reads per tap instead of 2 reads + 2 multiplies) 0.111, every LDS read of a step issued before
// the first use 0.105, two barriers per step with single row buffers 0.097, IEEE divisions in P 0.101.
#ifndef GS_LOSS_SH
#define GS_LOSS_SH 52
#endif
#ifndef GS_LOSS_FT
#define GS_LOSS_FT 512
#endif
constexpr int FT = GS_LOSS_FT;      // threads = columns of the H1 / V1 / P stages
constexpr int FHALO = 3 * R;        // flat halo of one horizontal filter
constexpr int FCW = FT - 2 * FHALO; // output columns of a workgroup
constexpr int SH = GS_LOSS_SH;      // output rows of a workgroup

__global__ void __launch_bounds__(FT) loss_fused_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                        LossGeom L, Window Wd, float *__restrict__ grad,
                                                        float *__restrict__ p_ssim, float *__restrict__ p_l1) {
#define GS_LOSS_WEIGHTED 0
#include "loss_fused_body.inc"
#undef GS_LOSS_WEIGHTED
}

// gs_loss_l1_ssim_weighted: the same kernel with a per-pixel weight m [H, W] (finite, >= 0; the three channels of a pixel
// share it) on what that pixel contributes:
//   l1 = sum_p m_p sum_c |x - y|,  ssim = sum_{q interior} m_q sum_c S_qc,
//   dL/dx = a m sign(x - y) - b [ g*(m D_mu) + 2 x g*(m D_xx) + y g*(m D_xy) ]
// -- the weights sit in front of the second filter, so a thread needs the weight of its own pixel only (two 4-byte reads per
// step).  Multiplying by 1.0f is exact and the operation order is loss_fused_kernel's: an all-ones map gives its bits.
__global__ void __launch_bounds__(FT) loss_weighted_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ m, LossGeom L, Window Wd,
                                                           float *__restrict__ grad, float *__restrict__ p_ssim,
                                                           float *__restrict__ p_l1) {
#define GS_LOSS_WEIGHTED 1
#include "loss_fused_body.inc"
#undef GS_LOSS_WEIGHTED
}

// ssim_weight = 0: the L1 term alone (any image size)
constexpr int L1_BLOCKS = 1024;
__global__ void __launch_bounds__(256) l1_only_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                      int64_t n, float a, float *__restrict__ grad,
                                                      float *__restrict__ p_ssim, float *__restrict__ p_l1) {
    __shared__ float s_red[4];
    float l1_sum = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = x[i] - y[i];
        l1_sum += fabsf(d);
        grad[i] = a * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
    }
    const float tot = block_sum(l1_sum, s_red);
    if (threadIdx.x == 0) {
        p_ssim[blockIdx.x] = 0.f;
        p_l1[blockIdx.x] = tot;
    }
}

// ... with the weight map (element i belongs to pixel i / 3); l1_only_kernel's grid and order of sums
__global__ void __launch_bounds__(256) l1_weighted_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ m, int64_t n, float a,
                                                          float *__restrict__ grad, float *__restrict__ p_ssim,
                                                          float *__restrict__ p_l1) {
    __shared__ float s_red[4];
    float l1_sum = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = x[i] - y[i], mo = m[i / 3];
        l1_sum += mo * fabsf(d);
        grad[i] = mo > 0.f ? a * mo * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f) : 0.f;  // (+0.0 under a zero weight)
    }
    const float tot = block_sum(l1_sum, s_red);
    if (threadIdx.x == 0) {
        p_ssim[blockIdx.x] = 0.f;
        p_l1[blockIdx.x] = tot;
    }
}

// loss_out = (loss, l1 mean, ssim mean); w_ssim: the weight of the SSIM term -- w, or 0 where the term does not exist (a
// weighted loss whose interior weights sum to zero)
__global__ void __launch_bounds__(256) loss_finish_kernel(const float *__restrict__ p_ssim,
                                                          const float *__restrict__ p_l1, int n, float inv_l1,
                                                          float inv_ssim, float w, float w_ssim,
                                                          float *__restrict__ loss_out) {
    __shared__ float s_red[4];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        a += p_ssim[i];
        b += p_l1[i];
    }
    const float ssim = block_sum(a, s_red) * inv_ssim;
    __syncthreads();
    const float l1 = block_sum(b, s_red) * inv_l1;
    if (threadIdx.x == 0) {
        loss_out[0] = (1.f - w) * l1 + (w_ssim > 0.f ? w_ssim * (1.f - ssim) : 0.f);
        loss_out[1] = l1;
        loss_out[2] = w_ssim > 0.f ? ssim : 0.f;
    }
}

}  // namespace

static inline int64_t loss_blocks(int32_t H, int32_t W) {
    const int64_t fused = gs_div_up(3 * (int64_t)W, FCW) * gs_div_up(H, SH);
    return fused > L1_BLOCKS ? fused : L1_BLOCKS;
}

extern "C" size_t gs_loss_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return 2 * gs_align_up(sizeof(float) * loss_blocks(H, W), 256);
}

// torchmetrics _gaussian: exp(-(d / sigma)^2 / 2) in fp32, normalised by its fp32 sum
static inline Window loss_window() {
    Window Wd;
    float sum = 0.f;
    for (int k = 0; k < K; ++k) {
        const float d = (float)(k - R) / 1.5f;
        Wd.g[k] = expf(-(d * d) / 2.f);
        sum += Wd.g[k];
    }
    for (int k = 0; k < K; ++k) Wd.g[k] /= sum;
    return Wd;
}

// a = (1 - w) / n_l1 and b = w / n_ss in double, rounded once; a term whose normaliser is zero (a weighted loss whose
// weights sum to zero) has the coefficient zero
static inline LossGeom loss_geom(int32_t H, int32_t W, float ssim_weight, double n_l1, double n_ss) {
    LossGeom L;
    L.H = H;
    L.W = W;
    L.c1 = 0.01f * 0.01f;
    L.c2 = 0.03f * 0.03f;
    L.a = n_l1 > 0.0 ? (float)((1.0 - ssim_weight) / n_l1) : 0.f;
    L.b = n_ss > 0.0 ? (float)(ssim_weight / n_ss) : 0.f;
    return L;
}

extern "C" int gs_loss_l1_ssim(const float *pred, const float *target, int32_t H, int32_t W, float ssim_weight,
                               float *grad, float *loss_out, void *workspace, size_t workspace_bytes,
                               gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(pred && target && grad, "null pointer");
    GS_CHECK_ARG(ssim_weight >= 0.f && ssim_weight <= 1.f, "ssim_weight must be in [0, 1]");
    GS_CHECK_ARG(ssim_weight == 0.f || (H > 2 * R && W > 2 * R), "SSIM needs an image larger than its 11x11 window");
    GS_CHECK_ARG(workspace && workspace_bytes >= gs_loss_workspace_bytes(H, W), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *p_ssim = (float *)workspace;
    float *p_l1 = (float *)((char *)p_ssim + gs_align_up(sizeof(float) * loss_blocks(H, W), 256));
    const Window Wd = loss_window();
    const double n_l1 = 3.0 * H * W, n_ss = ssim_weight > 0.f ? 3.0 * (H - 2 * R) * (double)(W - 2 * R) : 1.0;
    const LossGeom L = loss_geom(H, W, ssim_weight, n_l1, n_ss);
    int64_t nb;
    if (ssim_weight > 0.f) {
        const dim3 grid((unsigned)gs_div_up(3 * (int64_t)W, FCW), (unsigned)gs_div_up(H, SH));
        nb = (int64_t)grid.x * grid.y;
        hipLaunchKernelGGL(loss_fused_kernel, grid, dim3(FT), 0, s, pred, target, L, Wd, grad, p_ssim, p_l1);
    } else {
        const int64_t n = 3 * (int64_t)H * W;
        nb = gs_div_up(n, 256 * 4) < L1_BLOCKS ? gs_div_up(n, 256 * 4) : L1_BLOCKS;
        hipLaunchKernelGGL(l1_only_kernel, dim3((unsigned)nb), dim3(256), 0, s, pred, target, n, L.a, grad, p_ssim, p_l1);
    }
    GS_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, p_ssim, p_l1, (int)nb, (float)(1.0 / n_l1),
                           (float)(1.0 / n_ss), ssim_weight, ssim_weight, loss_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int gs_loss_l1_ssim_weighted(const float *pred, const float *target, const float *weight, int32_t H, int32_t W,
                                        float ssim_weight, double weight_sum, double weight_sum_interior, float *grad,
                                        float *loss_out, void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(pred && target && weight && grad, "null pointer");
    GS_CHECK_ARG(ssim_weight >= 0.f && ssim_weight <= 1.f, "ssim_weight must be in [0, 1]");
    GS_CHECK_ARG(ssim_weight == 0.f || (H > 2 * R && W > 2 * R), "SSIM needs an image larger than its 11x11 window");
    GS_CHECK_ARG(weight_sum >= 0.0 && weight_sum <= 1.7976931348623157e308 && weight_sum_interior >= 0.0 &&
                     weight_sum_interior <= 1.7976931348623157e308,
                 "weight_sum and weight_sum_interior must be finite and not negative");
    GS_CHECK_ARG(workspace && workspace_bytes >= gs_loss_workspace_bytes(H, W), "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float *p_ssim = (float *)workspace;
    float *p_l1 = (float *)((char *)p_ssim + gs_align_up(sizeof(float) * loss_blocks(H, W), 256));
    // the SSIM term exists where it has a weight and interior pixels that carry one; without it the weighted L1 kernel runs
    const bool with_ssim = ssim_weight > 0.f && weight_sum_interior > 0.0;
    const double n_l1 = 3.0 * weight_sum, n_ss = with_ssim ? 3.0 * weight_sum_interior : 1.0;
    const LossGeom L = loss_geom(H, W, ssim_weight, n_l1, n_ss);  // (L.b is read by the SSIM kernel only)
    int64_t nb;
    if (with_ssim) {
        const Window Wd = loss_window();
        const dim3 grid((unsigned)gs_div_up(3 * (int64_t)W, FCW), (unsigned)gs_div_up(H, SH));
        nb = (int64_t)grid.x * grid.y;
        hipLaunchKernelGGL(loss_weighted_kernel, grid, dim3(FT), 0, s, pred, target, weight, L, Wd, grad, p_ssim, p_l1);
    } else {
        const int64_t n = 3 * (int64_t)H * W;
        nb = gs_div_up(n, 256 * 4) < L1_BLOCKS ? gs_div_up(n, 256 * 4) : L1_BLOCKS;
        hipLaunchKernelGGL(l1_weighted_kernel, dim3((unsigned)nb), dim3(256), 0, s, pred, target, weight, n, L.a, grad, p_ssim,
                           p_l1);
    }
    GS_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, s, p_ssim, p_l1, (int)nb,
                           n_l1 > 0.0 ? (float)(1.0 / n_l1) : 0.f, (float)(1.0 / n_ss), ssim_weight,
                           with_ssim ? ssim_weight : 0.f, loss_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}

