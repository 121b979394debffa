// seed.hip -- new Gaussians from an RGB-D frame by back-projection (gs_seed_classify / gs_seed_apply, include/gs_abi.h).
//
// A depth camera measured a range z at a pixel; the current model renders D = sum_i w_i d_i and A = sum_i w_i there (the maps
// of a GS_FRAME_AUX frame).  Every `stride`-th pixel in x and y (the LATTICE: x % stride == stride / 2, likewise y) that
// carries a measurement (z > 0 and finite, the rule of gs_loss_depth) and that the model does not explain --
//     no maps given   or   A < alpha_thresh   or   z A < (1 - front_rel) D      (the measurement lies in front of the expected
//                                                                               depth D / A by more than front_rel; no division)
// -- becomes one Gaussian at the measured point.  Three launches, in the manner of densify.hip:
//   S1 seed_classify_kernel : a thread per lattice pixel decides; the wave's ballot (8 bytes per 64 lattice pixels) and the
//                             workgroup's (selected, measured) counts go to the workspace;
//   S2 seed_scan_kernel     : exclusive scan of the workgroups' counts, totals -> counts_dev = (selected, measured);
//   S3 seed_apply_kernel    : a thread per lattice pixel again; a selected one has rank = its workgroup's offset + the bits of
//                             the earlier waves' ballots + the bits below its own lane, and writes row offset + rank.
// The rank of a pixel is the number of selected pixels before it in row-major order: the output order is a pure function of
// the inputs, no slot is claimed with an atomic, two runs give the same bytes.  Nothing is written when offset + selected
// exceeds `capacity` (counts_dev still holds the need: the convention of gs_densify_apply).
// A selected pixel (x, y), in fp32, one rounding per operation (the file is compiled with -ffp-contract=off):
//   u = (x + left - padW / 2 + 0.5) / fx,  v = (y + top - padH / 2 + 0.5) / fy     the renderer's own ray through the centre of
//                                                                   the pixel (raster_pixel_coord; gs_geometry.RayBasis)
//   gs_seed_apply_pp (a camera whose principal point is off the renderer's centre by (dx, dy) pixels, gs_seed_camera_pp): the
//   ray moves with it, u = fl(fl(fl((float)(x + left - padW / 2) + 0.5f) - dx) / fx), v likewise -- the pixel's ray of a
//   GS_FRAME_PRINCIPAL_POINT frame of that camera, so the Gaussian still projects onto the centre of its pixel.  A kernel of
//   its own (seed_apply_pp_kernel); gs_seed_apply's runs what it ran before.
//   z_cam = z / sqrt(u u + v v + 1),  p_c = (u z_cam, v z_cam, z_cam),  pos = rot^T (p_c - tran)
//   sigma = scale_factor stride z_cam / ((fx + fy) / 2): `scale_factor` lattice steps at that depth; stored as the inverse of
//           the renderer's activation (project_common.h `activate`): max(sigma - 1e-4, 0) for abs, log sigma for exp
//   quat = (1, 0, 0, 0),  opa = logit(opa_init),  colour: logit(clamp(c, 1 / 512, 1 - 1 / 512)) per channel (half an 8-bit step
//           away from 0 and 1: the logit stays within +-6.24); SH: DC = logit / 0.28209479 (utils.py:345-348), the rest zero.
// The SH rows (27 or 48 floats, all but three of them zero) are written by the whole wave: its selected pixels are consecutive
// rows, so the wave walks that run of floats lane by lane in whole lines, the DC values handed over through LDS.
#include <cfloat>
#include <cmath>

#include "gs_common.h"

namespace {

constexpr int SEED_BLOCK = 256, SEED_WAVES = SEED_BLOCK / 64;
constexpr float SEED_COLOR_MIN = 1.0f / 512.0f;
constexpr float SEED_SH_C0 = 0.28209479177387814f;

struct SeedLattice {
    int32_t W, stride, off, Lw;  // pixel (lx * stride + off, ly * stride + off) for lattice index ly * Lw + lx
    int64_t L;                   // lattice pixels
};

struct SeedApplyParams {
    float rot[9], tran[3], fx, fy;
    int32_t x0, y0;  // left - padW / 2, top - padH / 2: the padded-image pixel index minus half the padded size
    float k_sigma, f_mean, opa_logit;
    int32_t scale_act;
};

inline SeedLattice seed_lattice(int32_t H, int32_t W, int32_t stride) {
    SeedLattice G;
    G.W = W;
    G.stride = stride;
    G.off = stride / 2;
    G.Lw = W > G.off ? (W - G.off + stride - 1) / stride : 0;
    const int32_t Lh = H > G.off ? (H - G.off + stride - 1) / stride : 0;
    G.L = (int64_t)G.Lw * Lh;
    return G;
}

__device__ __forceinline__ int64_t seed_pixel(const SeedLattice &G, int64_t j, int32_t &x, int32_t &y) {
    const int32_t ly = (int32_t)(j / G.Lw), lx = (int32_t)(j - (int64_t)ly * G.Lw);
    x = lx * G.stride + G.off;
    y = ly * G.stride + G.off;
    return (int64_t)y * G.W + x;
}

__global__ void __launch_bounds__(SEED_BLOCK) seed_classify_kernel(const float *__restrict__ range,
                                                                  const float *__restrict__ depth,
                                                                  const float *__restrict__ alpha, SeedLattice G,
                                                                  float alpha_thresh, float front_keep,
                                                                  unsigned long long *__restrict__ masks,
                                                                  uint2 *__restrict__ block_counts) {
    __shared__ uint32_t s_sel[SEED_WAVES], s_meas[SEED_WAVES];
    const int64_t j = (int64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
    bool meas = false, sel = false;
    if (j < G.L) {
        int32_t x, y;
        const int64_t p = seed_pixel(G, j, x, y);
        const float z = range[p];
        meas = z > 0.f && z <= FLT_MAX;  // (false for NaN and +inf)
        if (meas) {
            if (depth == nullptr) {
                sel = true;
            } else {
                const float A = alpha[p], D = depth[p];
                sel = A < alpha_thresh || z * A < front_keep * D;
            }
        }
    }
    const unsigned long long ms = __ballot(sel), mm = __ballot(meas);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(size_t)blockIdx.x * SEED_WAVES + wave] = ms;
        s_sel[wave] = (uint32_t)__popcll(ms);
        s_meas[wave] = (uint32_t)__popcll(mm);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = make_uint2(s_sel[0] + s_sel[1] + s_sel[2] + s_sel[3], s_meas[0] + s_meas[1] + s_meas[2] + s_meas[3]);
}

// one workgroup: block_counts[i].x <- exclusive scan of the selected counts; counts = (selected, measured)
__global__ void __launch_bounds__(1024) seed_scan_kernel(uint2 *__restrict__ block_counts, int nblk,
                                                         long long *__restrict__ counts) {
    __shared__ uint32_t s_wave[2][16];
    __shared__ uint32_t s_carry[2];
    if (threadIdx.x < 2) s_carry[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + threadIdx.x;
        const uint2 v = i < nblk ? block_counts[i] : make_uint2(0, 0);
        const uint32_t incl = gs_wave_incl_scan_u32(v.x), meas = gs_wave_sum_u32(v.y);
        if (lane == 63) {
            s_wave[0][wave] = incl;
            s_wave[1][wave] = meas;
        }
        __syncthreads();
        uint32_t off = 0, t = 0, tm = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            off += w < wave ? s_wave[0][w] : 0;
            t += s_wave[0][w];
            tm += s_wave[1][w];
        }
        if (i < nblk) block_counts[i].x = s_carry[0] + off + incl - v.x;
        const uint32_t next = s_carry[0] + t, next_m = s_carry[1] + tm;
        __syncthreads();
        if (threadIdx.x == 0) {
            s_carry[0] = next;
            s_carry[1] = next_m;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = s_carry[0];
        counts[1] = s_carry[1];
    }
}

struct SeedOut {
    float *pos, *quat, *scale, *opa, *rgb;
};

// (one body, two kernels: seed_apply_body.inc)
template <int CD>
__global__ void __launch_bounds__(SEED_BLOCK) seed_apply_kernel(const float *__restrict__ image,
                                                               const float *__restrict__ range, SeedLattice G,
                                                               SeedApplyParams P, SeedOut O, int64_t offset, int64_t capacity,
                                                               const unsigned long long *__restrict__ masks,
                                                               const uint2 *__restrict__ block_offsets,
                                                               const long long *__restrict__ counts) {
    constexpr bool PP = false;
    constexpr float pp_dx = 0.f, pp_dy = 0.f;
#include "seed_apply_body.inc"
}
// gs_seed_apply_pp: the camera's principal point is off the renderer's centre by (pp_dx, pp_dy) pixels; the ray moves with it
template <int CD>
__global__ void __launch_bounds__(SEED_BLOCK) seed_apply_pp_kernel(const float *__restrict__ image,
                                                                  const float *__restrict__ range, SeedLattice G,
                                                                  SeedApplyParams P, float pp_dx, float pp_dy, SeedOut O,
                                                                  int64_t offset, int64_t capacity,
                                                                  const unsigned long long *__restrict__ masks,
                                                                  const uint2 *__restrict__ block_offsets,
                                                                  const long long *__restrict__ counts) {
    constexpr bool PP = true;
#include "seed_apply_body.inc"
}

struct SeedWs {
    unsigned long long *masks;
    uint2 *block_counts;
    size_t bytes;
};
// sized for stride 1 (every pixel a lattice pixel): one size per image, whatever the stride of the call
SeedWs seed_carve(void *base, int64_t n) {
    SeedWs w;
    const int64_t nblk = gs_div_up(n > 0 ? n : 1, SEED_BLOCK);
    const size_t a = gs_align_up(sizeof(unsigned long long) * SEED_WAVES * (size_t)nblk, 256);
    w.masks = (unsigned long long *)base;
    w.block_counts = base ? (uint2 *)((char *)base + a) : nullptr;
    w.bytes = a + gs_align_up(sizeof(uint2) * (size_t)nblk, 256);
    return w;
}

int seed_check_opts(const gs_seed_opts *o) {
    GS_CHECK_ARG(o != nullptr, "opts is null");
    GS_CHECK_ARG(o->stride >= 1, "stride must be >= 1");
    GS_CHECK_ARG(o->scale_activation == 0 || o->scale_activation == 1, "scale_activation must be 0 (abs) or 1 (exp)");
    GS_CHECK_ARG(o->color_dim == 3 || o->color_dim == 27 || o->color_dim == 48, "color_dim must be 3, 27 or 48");
    GS_CHECK_ARG(o->opa_init > 0.f && o->opa_init < 1.f, "opa_init must lie in (0, 1)");
    GS_CHECK_ARG(o->scale_factor > 0.f && std::isfinite(o->scale_factor), "scale_factor must be positive and finite");
    GS_CHECK_ARG(std::isfinite(o->alpha_thresh) && std::isfinite(o->front_rel), "alpha_thresh and front_rel must be finite");
    return 0;
}

}  // namespace

extern "C" size_t gs_seed_workspace_bytes(int32_t H, int32_t W) {
    return H < 0 || W < 0 ? 0 : seed_carve(nullptr, (int64_t)H * W).bytes;
}

extern "C" int gs_seed_classify(const float *range, const float *depth, const float *alpha, int32_t H, int32_t W,
                                const gs_seed_opts *opts, int64_t *counts_dev, void *workspace, size_t workspace_bytes,
                                gs_stream_t stream) {
    int rc = seed_check_opts(opts);
    if (rc) return rc;
    GS_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "image size out of range");
    GS_CHECK_ARG(range != nullptr, "range is null");
    GS_CHECK_ARG((depth == nullptr) == (alpha == nullptr), "the depth and alpha maps come both or neither");
    GS_CHECK_ARG(counts_dev != nullptr, "counts_dev is null");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_seed_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const SeedLattice G = seed_lattice(H, W, opts->stride);
    const SeedWs w = seed_carve(workspace, (int64_t)H * W);
    const int nblk = (int)gs_div_up(G.L, SEED_BLOCK);
    if (nblk > 0) {
        hipLaunchKernelGGL(seed_classify_kernel, dim3(nblk), dim3(SEED_BLOCK), 0, s, range, depth, alpha, G,
                           opts->alpha_thresh, 1.0f - opts->front_rel, w.masks, w.block_counts);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(seed_scan_kernel, dim3(1), dim3(1024), 0, s, w.block_counts, nblk, (long long *)counts_dev);
    GS_CHECK_LAUNCH();
    return 0;
}

// gs_seed_apply (pp = nullptr) and gs_seed_apply_pp (pp = the two offsets; (0, 0) runs gs_seed_apply's kernel)
static int gs_seed_apply_impl(const float *image, const float *range, const gs_seed_camera *cam, const float *pp,
                           const gs_seed_opts *opts, float *pos, float *quat, float *scale, float *opa, float *rgb,
                           int64_t offset, int64_t capacity, const int64_t *counts_dev, const void *workspace,
                           size_t workspace_bytes, gs_stream_t stream) {
    int rc = seed_check_opts(opts);
    if (rc) return rc;
    GS_CHECK_ARG(cam != nullptr, "camera is null");
    const int32_t H = cam->height, W = cam->width;
    GS_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), "image size out of range");
    GS_CHECK_ARG(cam->focal_x > 0.f && cam->focal_y > 0.f && std::isfinite(cam->focal_x) && std::isfinite(cam->focal_y),
                 "focal lengths must be positive and finite");
    GS_CHECK_ARG(image != nullptr && range != nullptr, "image or range is null");
    GS_CHECK_ARG(offset >= 0 && capacity >= 0, "offset and capacity must not be negative");
    GS_CHECK_ARG(counts_dev != nullptr, "counts_dev is null");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= gs_seed_workspace_bytes(H, W),
                 "workspace null, misaligned or too small");
    if (capacity <= offset) return 0;  // no row can be written (the caller saw selected == 0, or the arrays are full)
    GS_CHECK_ARG(pos && quat && scale && opa && rgb, "null output");
    GS_CHECK_ARG(((uintptr_t)quat & 15) == 0, "quat must be 16-byte aligned");
    const SeedLattice G = seed_lattice(H, W, opts->stride);
    const int nblk = (int)gs_div_up(G.L, SEED_BLOCK);
    if (nblk == 0) return 0;
    SeedApplyParams P;
    for (int k = 0; k < 9; ++k) P.rot[k] = cam->rot[k];
    for (int k = 0; k < 3; ++k) P.tran[k] = cam->tran[k];
    P.fx = cam->focal_x;
    P.fy = cam->focal_y;
    const int32_t padW = (W + GS_TILE - 1) / GS_TILE * GS_TILE, padH = (H + GS_TILE - 1) / GS_TILE * GS_TILE;
    P.x0 = (padW - W) / 2 - padW / 2;  // the centred crop of the padded image (splatter.py:267-272)
    P.y0 = (padH - H) / 2 - padH / 2;
    P.k_sigma = opts->scale_factor * (float)opts->stride;
    P.f_mean = (cam->focal_x + cam->focal_y) * 0.5f;
    P.opa_logit = (float)(-log(1.0 / (double)opts->opa_init - 1.0));  // inverse_sigmoid, utils.py:350-351
    P.scale_act = opts->scale_activation;
    const SeedWs w = seed_carve(const_cast<void *>(workspace), (int64_t)H * W);
    const SeedOut O = {pos, quat, scale, opa, rgb};
    hipStream_t s = (hipStream_t)stream;
    const long long *cnt = (const long long *)counts_dev;
    const bool off_centre = pp && (pp[0] != 0.f || pp[1] != 0.f);
    gs_for_color_dim(opts->color_dim, [&](auto cd) {
        if (off_centre)
            hipLaunchKernelGGL(seed_apply_pp_kernel<decltype(cd)::value>, dim3(nblk), dim3(SEED_BLOCK), 0, s, image, range, G, P,
                               pp[0], pp[1], O, offset, capacity, w.masks, w.block_counts, cnt);
        else
            hipLaunchKernelGGL(seed_apply_kernel<decltype(cd)::value>, dim3(nblk), dim3(SEED_BLOCK), 0, s, image, range, G, P, O,
                               offset, capacity, w.masks, w.block_counts, cnt);
    });
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_seed_apply(const float *image, const float *range, const gs_seed_camera *cam, const gs_seed_opts *opts,
                             float *pos, float *quat, float *scale, float *opa, float *rgb, int64_t offset,
                             int64_t capacity, const int64_t *counts_dev, const void *workspace, size_t workspace_bytes,
                             gs_stream_t stream) {
    return gs_seed_apply_impl(image, range, cam, nullptr, opts, pos, quat, scale, opa, rgb, offset, capacity, counts_dev, workspace,
                           workspace_bytes, stream);
}

extern "C" int gs_seed_apply_pp(const float *image, const float *range, const gs_seed_camera_pp *cam, const gs_seed_opts *opts,
                                float *pos, float *quat, float *scale, float *opa, float *rgb, int64_t offset,
                                int64_t capacity, const int64_t *counts_dev, const void *workspace, size_t workspace_bytes,
                                gs_stream_t stream) {
    GS_CHECK_ARG(cam != nullptr, "camera is null");
    GS_CHECK_ARG(std::isfinite(cam->pp_dx) && std::isfinite(cam->pp_dy), "the principal point's offset must be finite");
    const float pp[2] = {cam->pp_dx, cam->pp_dy};
    return gs_seed_apply_impl(image, range, &cam->cam, pp, opts, pos, quat, scale, opa, rgb, offset, capacity, counts_dev,
                           workspace, workspace_bytes, stream);
}
