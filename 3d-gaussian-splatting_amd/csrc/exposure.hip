// exposure.hip -- a view's affine exposure, gain[3] and bias[3] per colour channel, around any of the colour losses
// (gs_exposure_apply, gs_exposure_backward, gs_exposure_workspace_bytes; include/gs_abi.h).
//
//   apply    :  I'_pc = fl(fl(gain_c I_pc) + bias_c)                       one streaming pass, one launch
//   backward :  g_pc  = fl(gain_c g'_pc) in place of g' = dL/dI',          one streaming pass +
//               dL/dgain_c = sum_p g'_pc I_pc,  dL/dbias_c = sum_p g'_pc   one workgroup that adds the rows, rounds each sum
//                                                                          to fp32 once and, with `adam`, steps the six numbers
// The file is built with -ffp-contract=off: every product is rounded before it is added, so tests/exposure_ref.py -- numpy
// float32 for the maps, Python floats for the step -- follows it operation by operation; sqrt and pow alone are each
// library's own.  The six numbers are read from device memory when the kernels run.  The step is a second launch: every
// workgroup of the first has read the gain before the one workgroup of the second replaces it, and nothing reads it after.
// Four pixels (twelve floats, three 16-byte accesses) per lane and 1,024 pixels per workgroup with no grid cap, as
// map_loss.hip.  The sums: each product in double from its two fp32 operands (exact: 48 significant bits), per thread in
// pixel order, then the fixed-order sum of gs_common.h in double -> one row of six doubles per workgroup; the second launch
// adds the rows in double in the same order.  No atomics: bitwise repeatable.
#include <cmath>

#include "gs_common.h"

namespace {

static_assert(sizeof(gs_exposure_state) == 104, "the device state is 13 doubles");

constexpr int EX_BLOCK = 256, EX_PER_BLOCK = EX_BLOCK * 4;

inline int64_t exposure_blocks(int64_t H, int64_t W) { return (H * W + EX_PER_BLOCK - 1) / EX_PER_BLOCK; }

// the twelve floats of four consecutive pixels: element j belongs to channel j % 3
struct ex12 {
    float v[12];
};
__device__ __forceinline__ ex12 ex_load(const float *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 a = q[0], b = q[1], c = q[2];
    return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
}
__device__ __forceinline__ void ex_store(float *p, const ex12 &x) {
    float4 *q = reinterpret_cast<float4 *>(p);
    q[0] = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
    q[1] = make_float4(x.v[4], x.v[5], x.v[6], x.v[7]);
    q[2] = make_float4(x.v[8], x.v[9], x.v[10], x.v[11]);
}

__global__ void __launch_bounds__(EX_BLOCK)
    exposure_apply_kernel(const float *__restrict__ image, const float *__restrict__ exposure, int64_t n, float *__restrict__ out) {
    const int64_t i0 = ((int64_t)blockIdx.x * EX_BLOCK + threadIdx.x) * 4;
    if (i0 >= n) return;
    const float gain[3] = {exposure[0], exposure[1], exposure[2]}, bias[3] = {exposure[3], exposure[4], exposure[5]};
    if (i0 + 4 <= n) {
        ex12 x = ex_load(image + i0 * 3);
#pragma unroll
        for (int j = 0; j < 12; ++j) x.v[j] = gain[j % 3] * x.v[j] + bias[j % 3];  // (two roundings: -ffp-contract=off)
        ex_store(out + i0 * 3, x);
    } else {
        for (int64_t e = i0 * 3; e < n * 3; ++e)  // the up to three pixels an image whose size is no multiple of four ends with
            out[e] = gain[e % 3] * image[e] + bias[e % 3];
    }
}

// SUMS: also this workgroup's row of the six sums (gain 0..2, bias 0..2) -> part[6 blockIdx.x ..]
template <bool SUMS>
__global__ void __launch_bounds__(EX_BLOCK)
    exposure_backward_kernel(const float *__restrict__ image, float *grad, const float *__restrict__ exposure, int64_t n,
                             double *__restrict__ part) {
    __shared__ double s_w[EX_BLOCK / 64][6];
    const int64_t i0 = ((int64_t)blockIdx.x * EX_BLOCK + threadIdx.x) * 4;
    const float gain[3] = {exposure[0], exposure[1], exposure[2]};
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i0 + 4 <= n) {
        ex12 g = ex_load(grad + i0 * 3);
        if (SUMS) {
            const ex12 x = ex_load(image + i0 * 3);
#pragma unroll
            for (int j = 0; j < 12; ++j) {  // (pixel order within a channel)
                acc[j % 3] += (double)g.v[j] * (double)x.v[j];
                acc[3 + j % 3] += (double)g.v[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) g.v[j] = gain[j % 3] * g.v[j];
        ex_store(grad + i0 * 3, g);
    } else {
        for (int64_t e = i0 * 3; e < n * 3; ++e) {  // the up to three tail pixels, in the same order
            const float gp = grad[e];
            const int c = (int)(e % 3);
            if (SUMS) {
                acc[c] += (double)gp * (double)image[e];
                acc[3 + c] += (double)gp;
            }
            grad[e] = gain[c] * gp;
        }
    }
    if (!SUMS) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_w[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 6)
        part[(int64_t)blockIdx.x * 6 + threadIdx.x] =
            ((s_w[0][threadIdx.x] + s_w[1][threadIdx.x]) + s_w[2][threadIdx.x]) + s_w[3][threadIdx.x];
}

struct ExposureAdamArgs {
    double lr[6], b1, b2, eps;
};

__device__ __forceinline__ bool ex_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (false for NaN)

// the rows added as depth_loss_finalize_kernel adds them (thread t takes rows t, t + 1024, ... in ascending order, the
// butterfly, the 16 waves in index order), each total rounded to fp32 once; then, with a state, one Adam step by thread 0
__global__ void __launch_bounds__(1024)
    exposure_finalize_kernel(const double *__restrict__ part, int64_t nrows, float *__restrict__ grad_out,
                             gs_exposure_state *__restrict__ state, const unsigned long long *__restrict__ skip_if_nonzero,
                             ExposureAdamArgs a, float *__restrict__ exposure) {
    __shared__ double s_w[16][6];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = threadIdx.x; r < nrows; r += 1024) {
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += part[r * 6 + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_w[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float g32[6];
    bool ok = true;
    for (int k = 0; k < 6; ++k) {
        double t = s_w[0][k];
        for (int w = 1; w < 16; ++w) t += s_w[w][k];
        g32[k] = (float)t;
        ok = ok && ex_finite(g32[k]);
        if (grad_out) grad_out[k] = g32[k];
    }
    if (!state) return;
    if (skip_if_nonzero != nullptr && *skip_if_nonzero != 0ull) return;  // the frame overflowed: nothing moves
    if (!ok) return;                                                    // a sum that is not finite: nothing moves
    // Adam on the fp32 gradients just written, in double (pose_step.hip's statement of it)
    const double steps = state->steps + 1.0;
    state->steps = steps;
    const double bc1 = 1.0 - pow(a.b1, steps), bc2 = 1.0 - pow(a.b2, steps);
    for (int k = 0; k < 6; ++k) {
        const double g = (double)g32[k];
        const double m = a.b1 * state->m[k] + (1.0 - a.b1) * g;
        const double v = a.b2 * state->v[k] + ((1.0 - a.b2) * g) * g;
        state->m[k] = m;
        state->v[k] = v;
        const double d = (a.lr[k] * (m / bc1)) / (sqrt(v / bc2) + a.eps);
        exposure[k] = (float)((double)exposure[k] - d);
    }
}

bool ex_rate(double x) { return x >= 0.0 && std::isfinite(x); }  // (false for NaN)

}  // namespace

extern "C" size_t gs_exposure_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return gs_align_up(sizeof(double) * 6 * (size_t)exposure_blocks(H, W), 256);
}

extern "C" int gs_exposure_apply(const float *image, const float *exposure_dev, int32_t H, int32_t W, float *out,
                                 gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(image && exposure_dev && out, "null pointer");
    GS_CHECK_ARG((((uintptr_t)image | (uintptr_t)out) & 15) == 0, "the maps must be 16-byte aligned");
    GS_CHECK_ARG(((uintptr_t)exposure_dev & 3) == 0, "exposure_dev must be 4-byte aligned");
    const int64_t n = (int64_t)H * W, blocks = exposure_blocks(H, W);
    GS_CHECK_ARG(blocks <= 0x7fffffff, "image size beyond 2^41 pixels");
    {  // the backward needs I: out may not overlap image
        const uintptr_t a = (uintptr_t)image, b = (uintptr_t)out, bytes = (uintptr_t)n * 12;
        GS_CHECK_ARG(a + bytes <= b || b + bytes <= a, "out may not alias image");
    }
    hipLaunchKernelGGL(exposure_apply_kernel, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, (hipStream_t)stream, image,
                       exposure_dev, n, out);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_exposure_backward(const float *image, float *grad, float *exposure_dev, int32_t H, int32_t W,
                                    float *grad_exposure_out, const gs_exposure_adam *adam, void *workspace,
                                    size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(image && grad && exposure_dev, "null pointer (only grad_exposure_out and adam may be NULL)");
    GS_CHECK_ARG((((uintptr_t)image | (uintptr_t)grad) & 15) == 0, "the maps must be 16-byte aligned");
    GS_CHECK_ARG((((uintptr_t)exposure_dev | (uintptr_t)grad_exposure_out) & 3) == 0,
                 "exposure_dev and grad_exposure_out must be 4-byte aligned");
    const int64_t n = (int64_t)H * W, blocks = exposure_blocks(H, W);
    GS_CHECK_ARG(blocks <= 0x7fffffff, "image size beyond 2^41 pixels");
    {
        const uintptr_t a = (uintptr_t)image, b = (uintptr_t)grad, bytes = (uintptr_t)n * 12;
        GS_CHECK_ARG(a + bytes <= b || b + bytes <= a, "grad may not alias image");
    }
    ExposureAdamArgs args = {};
    if (adam) {
        GS_CHECK_ARG(adam->state != nullptr, "adam: state is null");
        GS_CHECK_ARG((((uintptr_t)adam->state | (uintptr_t)adam->skip_if_nonzero) & 7) == 0,
                     "adam: state and skip_if_nonzero must be 8-byte aligned");
        GS_CHECK_ARG(ex_rate(adam->lr_gain) && ex_rate(adam->lr_bias) && ex_rate(adam->lr_scale),
                     "adam: lr_gain, lr_bias and lr_scale must not be negative, NaN or infinite");
        GS_CHECK_ARG(ex_rate(adam->eps), "adam: eps must not be negative, NaN or infinite");
        GS_CHECK_ARG(adam->beta1 >= 0.0 && adam->beta1 < 1.0 && adam->beta2 >= 0.0 && adam->beta2 < 1.0,
                     "adam: betas must lie in [0, 1)");
        for (int k = 0; k < 6; ++k) args.lr[k] = (k < 3 ? adam->lr_gain : adam->lr_bias) * adam->lr_scale;
        args.b1 = adam->beta1;
        args.b2 = adam->beta2;
        args.eps = adam->eps;
    }
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_exposure_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    double *part = (double *)workspace;
    if (!grad_exposure_out && !adam) {  // nobody reads the sums: the scaling alone
        hipLaunchKernelGGL(exposure_backward_kernel<false>, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, s, image, grad,
                           (const float *)exposure_dev, n, part);
        GS_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(exposure_backward_kernel<true>, dim3((unsigned)blocks), dim3(EX_BLOCK), 0, s, image, grad,
                       (const float *)exposure_dev, n, part);
    GS_CHECK_LAUNCH();
    hipLaunchKernelGGL(exposure_finalize_kernel, dim3(1), dim3(1024), 0, s, (const double *)part, blocks, grad_exposure_out,
                       adam ? (gs_exposure_state *)adam->state : nullptr,
                       adam ? (const unsigned long long *)adam->skip_if_nonzero : nullptr, args, exposure_dev);
    GS_CHECK_LAUNCH();
    return 0;
}
