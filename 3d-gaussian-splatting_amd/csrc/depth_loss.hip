// depth_loss.hip -- L1 depth supervision on the maps of a GS_FRAME_AUX frame (gs_loss_depth, include/gs_abi.h).
//
// The frame renders D = sum_i w_i d_i and A = sum_i w_i per pixel (d_i = |p_c|, the RANGE from the camera centre); the
// target z is a measured range per pixel, "no measurement" where it is <= 0, infinite or NaN.  Two residuals:
//   mode 0:  r = D - A z  (= sum_i w_i (d_i - z): no division, defined everywhere),   dr/dD = 1,      dr/dA = -z
//   mode 1:  r = D / A - z  (the expected depth), only where A >= alpha_min,           dr/dD = 1 / A,  dr/dA = -D / A^2
//   loss = scale sum_valid |r|,   grad_depth = scale sign(r) dr/dD,   grad_alpha = scale sign(r) dr/dA,
// zero gradients at pixels that do not count.  The caller folds weight / n_valid into `scale` (the target's valid pixels
// are known when the target is loaded): no count pass, no host synchronisation.
// One streaming pass: a lane takes four consecutive pixels (three 16-byte loads, two 16-byte stores: every wave
// instruction moves whole kilobyte runs), 1,024 pixels per workgroup.  The loss value: per-thread sums of |r| in pixel
// order, a fixed butterfly over the wave, the waves in index order -> one (sum, count) per workgroup; a one-workgroup
// kernel adds those in double in a fixed order (as pose_grad_finalize_kernel, cull_project.hip).  No atomics: bitwise
// repeatable.
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int DL_BLOCK = 256, DL_PER_BLOCK = DL_BLOCK * 4;

inline int64_t depth_loss_blocks(int64_t H, int64_t W) { return (H * W + DL_PER_BLOCK - 1) / DL_PER_BLOCK; }

// one pixel: returns |r| (0 where the pixel does not count) and its two gradients; `cnt` counts the pixels that counted
template <int MODE>
__device__ __forceinline__ float depth_loss_pixel(float D, float A, float z, float alpha_min, float scale, float &gD, float &gA,
                                                  uint32_t &cnt) {
    gD = 0.f;
    gA = 0.f;
    bool ok = z > 0.f && z <= 3.402823466e38f;  // (false for NaN and +inf)
    if (MODE == 1) ok = ok && A >= alpha_min;
    if (!ok) return 0.f;
    ++cnt;
    float r, dD, dA;
    if (MODE == 0) {
        r = D - A * z;
        dD = 1.f;
        dA = -z;
    } else {
        const float e = D / A;
        r = e - z;
        dD = 1.f / A;
        dA = -(e / A);
    }
    const float sg = r > 0.f ? scale : (r < 0.f ? -scale : 0.f);
    gD = sg * dD;
    gA = sg * dA;
    return fabsf(r);
}

template <int MODE>
__global__ void __launch_bounds__(DL_BLOCK) depth_loss_kernel(const float *__restrict__ depth, const float *__restrict__ alpha,
                                                             const float *__restrict__ target, int64_t n, float alpha_min,
                                                             float scale, float *__restrict__ grad_depth,
                                                             float *__restrict__ grad_alpha, float2 *__restrict__ part) {
    __shared__ float s_sum[DL_BLOCK / 64];
    __shared__ uint32_t s_cnt[DL_BLOCK / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * DL_BLOCK + threadIdx.x) * 4;
    float acc = 0.f;
    uint32_t cnt = 0;
    if (i0 + 4 <= n) {
        const float4 d = *reinterpret_cast<const float4 *>(depth + i0), a = *reinterpret_cast<const float4 *>(alpha + i0);
        const float4 z = *reinterpret_cast<const float4 *>(target + i0);
        float4 gd, ga;
        acc += depth_loss_pixel<MODE>(d.x, a.x, z.x, alpha_min, scale, gd.x, ga.x, cnt);
        acc += depth_loss_pixel<MODE>(d.y, a.y, z.y, alpha_min, scale, gd.y, ga.y, cnt);
        acc += depth_loss_pixel<MODE>(d.z, a.z, z.z, alpha_min, scale, gd.z, ga.z, cnt);
        acc += depth_loss_pixel<MODE>(d.w, a.w, z.w, alpha_min, scale, gd.w, ga.w, cnt);
        *reinterpret_cast<float4 *>(grad_depth + i0) = gd;
        *reinterpret_cast<float4 *>(grad_alpha + i0) = ga;
    } else {
        for (int64_t i = i0; i < n; ++i) {  // the up to three pixels an image whose size is no multiple of four ends with
            float gd, ga;
            acc += depth_loss_pixel<MODE>(depth[i], alpha[i], target[i], alpha_min, scale, gd, ga, cnt);
            grad_depth[i] = gd;
            grad_alpha[i] = ga;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = acc;
        s_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0)  // (a count is at most 1,024: exact as a float)
        part[blockIdx.x] = make_float2(((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3],
                                       (float)(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]));
}

// (loss, pixels that counted) = (scale x the sum of the workgroups' sums, the sum of their counts): thread t takes rows
// t, t + 1024, ... in ascending order, then a butterfly over the wave, then the waves in index order -- in double.
__global__ void __launch_bounds__(1024) depth_loss_finalize_kernel(const float2 *__restrict__ part, int64_t nrows, float scale,
                                                                   float *__restrict__ loss_out) {
    __shared__ double s_w[16][2];
    double a = 0.0, c = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += 1024) {
        const float2 v = part[r];
        a += (double)v.x;
        c += (double)v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6][0] = a;
        s_w[threadIdx.x >> 6][1] = c;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = s_w[0][threadIdx.x];
        for (int w = 1; w < 16; ++w) t += s_w[w][threadIdx.x];
        loss_out[threadIdx.x] = threadIdx.x == 0 ? (float)((double)scale * t) : (float)t;
    }
}

}  // namespace

extern "C" size_t gs_loss_depth_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return gs_align_up(sizeof(float2) * (size_t)depth_loss_blocks(H, W), 256);
}

extern "C" int gs_loss_depth(const float *depth, const float *alpha, const float *target, int32_t H, int32_t W, int32_t mode,
                             float alpha_min, float scale, float *grad_depth, float *grad_alpha, float *loss_out,
                             void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (residual D - A z) or 1 (expected depth D / A - z)");
    GS_CHECK_ARG(depth && alpha && target && grad_depth && grad_alpha, "null pointer");
    GS_CHECK_ARG(mode == 0 || alpha_min > 0.f, "mode 1: alpha_min must be positive (the residual divides by alpha)");
    GS_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    {  // the kernel walks the maps float4 by float4
        const void *al[] = {depth, alpha, target, grad_depth, grad_alpha};
        for (const void *q : al) GS_CHECK_ARG(((uintptr_t)q & 15) == 0, "the maps must be 16-byte aligned");
    }
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_loss_depth_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W, blocks = depth_loss_blocks(H, W);
    float2 *part = (float2 *)workspace;
    if (mode == 0)
        hipLaunchKernelGGL(depth_loss_kernel<0>, dim3((unsigned)blocks), dim3(DL_BLOCK), 0, s, depth, alpha, target, n, alpha_min,
                           scale, grad_depth, grad_alpha, part);
    else
        hipLaunchKernelGGL(depth_loss_kernel<1>, dim3((unsigned)blocks), dim3(DL_BLOCK), 0, s, depth, alpha, target, n, alpha_min,
                           scale, grad_depth, grad_alpha, part);
    GS_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3(1), dim3(1024), 0, s, (const float2 *)part, blocks, scale, loss_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
