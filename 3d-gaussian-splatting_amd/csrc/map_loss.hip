// map_loss.hip -- the two losses on the maps of a GS_FRAME_AUX frame: L1 depth supervision (gs_loss_depth) and the
// per-iteration loss of camera tracking against a frozen map (gs_loss_track); include/gs_abi.h.
//
// The frame renders the image I, D = sum_i w_i d_i and A = sum_i w_i per pixel (d_i = |p_c|, the RANGE from the camera
// centre); the targets are an image T and a measured range z per pixel, "no measurement" where it is <= 0, infinite or NaN.
// gs_loss_depth, two residuals:
//   mode 0:  r = D - A z  (= sum_i w_i (d_i - z): no division, defined everywhere),   dr/dD = 1,      dr/dA = -z
//   mode 1:  r = D / A - z  (the expected depth), only where A >= alpha_min,           dr/dD = 1 / A,  dr/dA = -D / A^2
//   loss = scale sum_valid |r|,   grad_depth = scale sign(r) dr/dD,   grad_alpha = scale sign(r) dr/dA,
//   zero gradients at pixels that do not count.  The caller folds weight / n_valid into `scale` (the target's valid pixels
//   are known when the target is loaded): no count pass, no host synchronisation.
// gs_loss_track:
//   colour: a pixel counts iff A >= alpha_min (the silhouette of the map: what the map does not cover says nothing about
//           the pose);  term = cs sum_c |I_c - T_c|,  grad_image_c = +-cs by the sign of I_c - T_c (0 where equal);
//   depth : a pixel counts iff it counts for colour, is measured and, with r of mode 1, the gate is off (depth_gate <= 0)
//           or |r| <= depth_gate;  term = ds |r| with mode 1's gradients at scale ds -- the same function, bit for bit;
//   cs = fl(scale color_weight), ds = fl(scale depth_weight); every other gradient is an exact zero; the masks are constants.
// Each is one streaming pass: a lane takes four consecutive pixels (16-byte loads and stores: every wave instruction moves
// whole kilobyte runs), 1,024 pixels per workgroup, the up to three tail pixels one by one.  The values: per-thread sums in
// pixel order, then the fixed-order sum of gs_common.h -> one row per workgroup, (sum, count) for depth and (colour sum, depth
// sum, depth count, -) for tracking; a one-workgroup kernel adds the rows in double in the same order.  No atomics:
// bitwise repeatable.
#include <cmath>

#include "gs_common.h"
#include "map_terms.h"  // map_measured, map_signed, map_expected_residual, map_expected_grads

namespace {

constexpr int ML_BLOCK = 256, ML_PER_BLOCK = ML_BLOCK * 4;

inline int64_t map_loss_blocks(int64_t H, int64_t W) { return (H * W + ML_PER_BLOCK - 1) / ML_PER_BLOCK; }

// one pixel: returns |r| (0 where the pixel does not count) and its two gradients; `cnt` counts the pixels that counted
template <int MODE>
__device__ __forceinline__ float depth_loss_pixel(float D, float A, float z, float alpha_min, float scale, float &gD, float &gA,
                                                  uint32_t &cnt) {
    gD = 0.f;
    gA = 0.f;
    bool ok = map_measured(z);
    if (MODE == 1) ok = ok && A >= alpha_min;
    if (!ok) return 0.f;
    ++cnt;
    float r, dD, dA;
    if (MODE == 0) {
        r = D - A * z;
        dD = 1.f;
        dA = -z;
    } else {
        float e;
        r = map_expected_residual(D, A, z, e);
        map_expected_grads(1.f, e, A, dD, dA);  // (a product with 1.f is exact)
    }
    const float sg = map_signed(r, scale);
    gD = sg * dD;
    gA = sg * dA;
    return fabsf(r);
}

template <int MODE>
__global__ void __launch_bounds__(ML_BLOCK) depth_loss_kernel(const float *__restrict__ depth, const float *__restrict__ alpha,
                                                             const float *__restrict__ target, int64_t n, float alpha_min,
                                                             float scale, float *__restrict__ grad_depth,
                                                             float *__restrict__ grad_alpha, float2 *__restrict__ part) {
    __shared__ float s_sum[ML_BLOCK / 64];
    __shared__ uint32_t s_cnt[ML_BLOCK / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * ML_BLOCK + threadIdx.x) * 4;
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
// t, t + 1024, ... in ascending order, then the butterfly and the 16 waves in index order -- in double (gs_common.h).
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

struct track_sums {
    float colour, depth;
    uint32_t cnt;
};

// one pixel: its five gradients, and its share of the three sums
template <bool RANGE>
__device__ __forceinline__ void track_loss_pixel(float i0, float i1, float i2, float t0, float t1, float t2, float D, float A,
                                                 float z, float alpha_min, float cs, float ds, float gate, float &g0, float &g1,
                                                 float &g2, float &gD, float &gA, track_sums &acc) {
    g0 = g1 = g2 = gD = gA = 0.f;
    if (!(A >= alpha_min)) return;  // (false for NaN)
    const float d0 = i0 - t0, d1 = i1 - t1, d2 = i2 - t2;
    g0 = map_signed(d0, cs);
    g1 = map_signed(d1, cs);
    g2 = map_signed(d2, cs);
    acc.colour += (fabsf(d0) + fabsf(d1)) + fabsf(d2);
    if (!RANGE) return;
    if (!map_measured(z)) return;
    float e;
    const float r = map_expected_residual(D, A, z, e);
    if (gate > 0.f && !(fabsf(r) <= gate)) return;
    ++acc.cnt;
    const float sg = map_signed(r, ds);
    map_expected_grads(sg, e, A, gD, gA);
    acc.depth += fabsf(r);
}

template <bool RANGE>
__global__ void __launch_bounds__(ML_BLOCK)
    track_loss_kernel(const float *__restrict__ image, const float *__restrict__ depth, const float *__restrict__ alpha,
                      const float *__restrict__ target_image, const float *__restrict__ target_range, int64_t n, float alpha_min,
                      float cs, float ds, float gate, float *__restrict__ grad_image, float *__restrict__ grad_depth,
                      float *__restrict__ grad_alpha, float4 *__restrict__ part) {
    __shared__ float s_col[ML_BLOCK / 64], s_dep[ML_BLOCK / 64];
    __shared__ uint32_t s_cnt[ML_BLOCK / 64];
    const int64_t i0 = ((int64_t)blockIdx.x * ML_BLOCK + threadIdx.x) * 4;
    track_sums acc = {0.f, 0.f, 0u};
    if (i0 + 4 <= n) {
        const float4 d = *reinterpret_cast<const float4 *>(depth + i0), a = *reinterpret_cast<const float4 *>(alpha + i0);
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RANGE) z = *reinterpret_cast<const float4 *>(target_range + i0);
        const float4 *pi = reinterpret_cast<const float4 *>(image + i0 * 3);
        const float4 *pt = reinterpret_cast<const float4 *>(target_image + i0 * 3);
        const float4 ia = pi[0], ib = pi[1], ic = pi[2], ta = pt[0], tb = pt[1], tc = pt[2];
        float4 ga, gb, gc, gd, gal;  // (ga, gb, gc: the twelve colour gradients of the four pixels in memory order)
        track_loss_pixel<RANGE>(ia.x, ia.y, ia.z, ta.x, ta.y, ta.z, d.x, a.x, z.x, alpha_min, cs, ds, gate, ga.x, ga.y, ga.z,
                                gd.x, gal.x, acc);
        track_loss_pixel<RANGE>(ia.w, ib.x, ib.y, ta.w, tb.x, tb.y, d.y, a.y, z.y, alpha_min, cs, ds, gate, ga.w, gb.x, gb.y,
                                gd.y, gal.y, acc);
        track_loss_pixel<RANGE>(ib.z, ib.w, ic.x, tb.z, tb.w, tc.x, d.z, a.z, z.z, alpha_min, cs, ds, gate, gb.z, gb.w, gc.x,
                                gd.z, gal.z, acc);
        track_loss_pixel<RANGE>(ic.y, ic.z, ic.w, tc.y, tc.z, tc.w, d.w, a.w, z.w, alpha_min, cs, ds, gate, gc.y, gc.z, gc.w,
                                gd.w, gal.w, acc);
        float4 *po = reinterpret_cast<float4 *>(grad_image + i0 * 3);
        po[0] = ga;
        po[1] = gb;
        po[2] = gc;
        *reinterpret_cast<float4 *>(grad_depth + i0) = gd;
        *reinterpret_cast<float4 *>(grad_alpha + i0) = gal;
    } else {
        for (int64_t i = i0; i < n; ++i) {  // the up to three pixels an image whose size is no multiple of four ends with
            float g0, g1, g2, gd, ga;
            track_loss_pixel<RANGE>(image[i * 3], image[i * 3 + 1], image[i * 3 + 2], target_image[i * 3],
                                    target_image[i * 3 + 1], target_image[i * 3 + 2], depth[i], alpha[i],
                                    RANGE ? target_range[i] : 0.f, alpha_min, cs, ds, gate, g0, g1, g2, gd, ga, acc);
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
        acc.cnt += __shfl_xor(acc.cnt, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_col[threadIdx.x >> 6] = acc.colour;
        s_dep[threadIdx.x >> 6] = acc.depth;
        s_cnt[threadIdx.x >> 6] = acc.cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0)  // (a count is at most 1,024: exact as a float)
        part[blockIdx.x] = make_float4(((s_col[0] + s_col[1]) + s_col[2]) + s_col[3], ((s_dep[0] + s_dep[1]) + s_dep[2]) + s_dep[3],
                                       (float)(((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3]), 0.f);
}

// values_out = (loss, colour term, depth term, pixels that counted for depth), summed as in depth_loss_finalize_kernel
__global__ void __launch_bounds__(1024) track_loss_finalize_kernel(const float4 *__restrict__ part, int64_t nrows, float scale,
                                                                   float color_weight, float depth_weight,
                                                                   float *__restrict__ values_out) {
    __shared__ double s_w[16][3];
    double c = 0.0, d = 0.0, k = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += 1024) {
        const float4 v = part[r];
        c += (double)v.x;
        d += (double)v.y;
        k += (double)v.z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o, 64);
        d += __shfl_xor(d, o, 64);
        k += __shfl_xor(k, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6][0] = c;
        s_w[threadIdx.x >> 6][1] = d;
        s_w[threadIdx.x >> 6][2] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[3];
        for (int j = 0; j < 3; ++j) {
            t[j] = s_w[0][j];
            for (int w = 1; w < 16; ++w) t[j] += s_w[w][j];
        }
        const double colour = (double)scale * (double)color_weight * t[0], dep = (double)scale * (double)depth_weight * t[1];
        values_out[0] = (float)(colour + dep);
        values_out[1] = (float)colour;
        values_out[2] = (float)dep;
        values_out[3] = (float)t[2];
    }
}

}  // namespace

extern "C" size_t gs_loss_depth_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return gs_align_up(sizeof(float2) * (size_t)map_loss_blocks(H, W), 256);
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
    const int64_t n = (int64_t)H * W, blocks = map_loss_blocks(H, W);
    float2 *part = (float2 *)workspace;
    if (mode == 0)
        hipLaunchKernelGGL(depth_loss_kernel<0>, dim3((unsigned)blocks), dim3(ML_BLOCK), 0, s, depth, alpha, target, n, alpha_min,
                           scale, grad_depth, grad_alpha, part);
    else
        hipLaunchKernelGGL(depth_loss_kernel<1>, dim3((unsigned)blocks), dim3(ML_BLOCK), 0, s, depth, alpha, target, n, alpha_min,
                           scale, grad_depth, grad_alpha, part);
    GS_CHECK_LAUNCH();
    if (loss_out) {
        hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3(1), dim3(1024), 0, s, (const float2 *)part, blocks, scale, loss_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" size_t gs_loss_track_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return gs_align_up(sizeof(float4) * (size_t)map_loss_blocks(H, W), 256);
}

extern "C" int gs_loss_track(const float *image, const float *depth, const float *alpha, const float *target_image,
                             const float *target_range, int32_t H, int32_t W, float alpha_min, float color_weight,
                             float depth_weight, float depth_gate, float scale, float *grad_image, float *grad_depth,
                             float *grad_alpha, float *values_out, void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(H > 0 && W > 0, "empty image");
    GS_CHECK_ARG(image && depth && alpha && target_image && grad_image && grad_depth && grad_alpha,
                 "null pointer (only target_range and values_out may be NULL)");
    GS_CHECK_ARG(alpha_min > 0.f, "alpha_min must be positive (the expected depth divides by alpha)");
    GS_CHECK_ARG(color_weight >= 0.f && depth_weight >= 0.f, "color_weight and depth_weight must not be negative or NaN");
    GS_CHECK_ARG(std::isfinite(scale), "scale must be finite");
    {  // the kernel walks the maps float4 by float4
        const void *al[] = {image, depth, alpha, target_image, target_range, grad_image, grad_depth, grad_alpha};
        for (const void *q : al) GS_CHECK_ARG(((uintptr_t)q & 15) == 0, "the maps must be 16-byte aligned");
    }
    GS_CHECK_ARG(((uintptr_t)values_out & 3) == 0, "values_out must be 4-byte aligned");
    const int64_t n = (int64_t)H * W, blocks = map_loss_blocks(H, W);
    GS_CHECK_ARG(blocks <= 0x7fffffff, "image size beyond 2^41 pixels");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= gs_loss_track_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const float cs = scale * color_weight, ds = scale * depth_weight;  // (one rounding each: -ffp-contract=off)
    float4 *part = (float4 *)workspace;
    if (target_range)
        hipLaunchKernelGGL(track_loss_kernel<true>, dim3((unsigned)blocks), dim3(ML_BLOCK), 0, s, image, depth, alpha,
                           target_image, target_range, n, alpha_min, cs, ds, depth_gate, grad_image, grad_depth, grad_alpha, part);
    else
        hipLaunchKernelGGL(track_loss_kernel<false>, dim3((unsigned)blocks), dim3(ML_BLOCK), 0, s, image, depth, alpha,
                           target_image, target_range, n, alpha_min, cs, ds, depth_gate, grad_image, grad_depth, grad_alpha, part);
    GS_CHECK_LAUNCH();
    if (values_out) {
        hipLaunchKernelGGL(track_loss_finalize_kernel, dim3(1), dim3(1024), 0, s, (const float4 *)part, blocks, scale,
                           color_weight, depth_weight, values_out);
        GS_CHECK_LAUNCH();
    }
    return 0;
}
