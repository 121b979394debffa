// overlap.hip -- covisibility of an incoming RGB-D frame with a set of keyframes (gs_view_overlap, include/gs_abi.h).
//
// Of the surface points the frame measured on its `stride` lattice (the lattice of gs_seed), how many does each view see?
// overlap_point.h states the decision for one point and one view; this file counts.  Two launches, no atomics:
//   O1 overlap_count_kernel    : a 256-thread workgroup takes a run of consecutive lattice pixels in row-major order, 256 at a
//                                time, a thread per pixel: the thread back-projects its pixel once and keeps the world point
//                                in three registers.  The view loop is uniform across the wave: a view's 64-byte row comes
//                                through uniform (scalar) loads of the device table, every lane decides its point, and the
//                                view costs one ballot and one popcount per wave.  View k's running count lives in lane
//                                k % 64 of register k / 64 -- four registers hold all 256.  At the end the four waves' counts
//                                meet in LDS and the workgroup writes its n_views + 2 partial counts (views, measured,
//                                measured and seen by nobody) as one row of uint32 in the workspace.
//   O2 overlap_finalize_kernel : a workgroup per 64 columns of those rows: four waves add rows r = w, w + 4, ... in ascending
//                                order in int64, the four sums are added in wave order -> counts_dev.
// Every row of the workspace that O2 reads was written whole by O1 in the same call: the result is a pure function of the
// inputs whatever the workspace held, and integer sums have no order to depend on.  A wave none of whose 64 pixels carries a
// measurement skips the view loop.
#include <cmath>

#include "gs_common.h"
#include "overlap_point.h"

namespace {

constexpr int OVL_BLOCK = 256, OVL_WAVES = OVL_BLOCK / 64;
constexpr int OVL_GROUPS = GS_OVERLAP_MAX_VIEWS / 64;  // registers of lane-distributed counts
constexpr int OVL_MAX_BLOCKS = 2048;                   // 8 workgroups on each of 256 CUs: longer runs beyond that
static_assert(GS_OVERLAP_MAX_VIEWS % 64 == 0, "counts are kept 64 views to a register");

struct OverlapLattice {
    int32_t W, stride, off, Lw;  // pixel (lx * stride + off, ly * stride + off) for lattice index ly * Lw + lx
    int64_t L;                   // lattice pixels
    int32_t chunks_per_block;    // a workgroup's run: this many chunks of 256 lattice pixels
};

struct OverlapPlan {
    OverlapLattice G;
    int32_t nblk;  // workgroups of O1 = rows of the workspace
};

inline OverlapPlan overlap_plan(int32_t H, int32_t W, int32_t stride) {
    OverlapPlan P;
    OverlapLattice &G = P.G;
    G.W = W;
    G.stride = stride;
    G.off = stride / 2;
    G.Lw = W > G.off ? (W - G.off + stride - 1) / stride : 0;
    const int32_t Lh = H > G.off ? (H - G.off + stride - 1) / stride : 0;
    G.L = (int64_t)G.Lw * Lh;
    const int64_t chunks = gs_div_up(G.L, OVL_BLOCK);
    G.chunks_per_block = (int32_t)(chunks > OVL_MAX_BLOCKS ? gs_div_up(chunks, OVL_MAX_BLOCKS) : 1);
    P.nblk = (int32_t)gs_div_up(chunks, G.chunks_per_block);
    return P;
}

// (one body, two kernels: overlap_count_body.inc.  PP: the frame's camera and the views carry principal-point offsets -- the
// frame's by value, view k's in row k of view_pp (two floats, uniform loads beside the view's 64-byte row; nullptr: no view
// has one) -- and the *_pp decisions of overlap_point.h are taken.)
__global__ void __launch_bounds__(OVL_BLOCK) __attribute__((amdgpu_num_sgpr(72))) overlap_count_kernel(const float *__restrict__ range, OverlapLattice G,
                                                                  gs_seed_camera cam,
                                                                  const gs_seed_camera *__restrict__ views, int32_t n_views,
                                                                  float near, int32_t border, uint32_t *__restrict__ rows) {
    constexpr bool PP = false;
    constexpr float cam_dx = 0.f, cam_dy = 0.f;
    constexpr const float2 *view_pp = nullptr;
#include "overlap_count_body.inc"
}
__global__ void __launch_bounds__(OVL_BLOCK) overlap_count_pp_kernel(const float *__restrict__ range, OverlapLattice G,
                                                                     gs_seed_camera_pp cam_pp,
                                                                     const gs_seed_camera *__restrict__ views,
                                                                     const float2 *__restrict__ view_pp, int32_t n_views,
                                                                     float near, int32_t border, uint32_t *__restrict__ rows) {
    constexpr bool PP = true;
    const gs_seed_camera &cam = cam_pp.cam;
    const float cam_dx = cam_pp.pp_dx, cam_dy = cam_pp.pp_dy;
#include "overlap_count_body.inc"
}

__global__ void __launch_bounds__(OVL_BLOCK) overlap_finalize_kernel(const uint32_t *__restrict__ rows, int32_t nblk,
                                                                     int32_t n_cols, long long *__restrict__ counts) {
    __shared__ long long s_sum[OVL_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    long long sum = 0;
    if (col < n_cols)
        for (int32_t r = wave; r < nblk; r += OVL_WAVES) sum += (long long)rows[(size_t)r * (size_t)n_cols + col];
    s_sum[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && col < n_cols) counts[col] = s_sum[0][lane] + s_sum[1][lane] + s_sum[2][lane] + s_sum[3][lane];
}

int overlap_check_opts(const gs_overlap_opts *o) {
    GS_CHECK_ARG(o != nullptr, "opts is null");
    GS_CHECK_ARG(o->stride >= 1, "stride must be >= 1");
    GS_CHECK_ARG(o->near > 0.f && std::isfinite(o->near), "near must be positive and finite");
    GS_CHECK_ARG(o->border >= 0, "border must not be negative");
    return 0;
}

int overlap_check_camera(const gs_seed_camera *c, const char *null_text) {
    GS_CHECK_ARG(c != nullptr, null_text);
    GS_CHECK_ARG(c->height > 0 && c->width > 0 && (int64_t)c->height * c->width < (1ll << 31), "image size out of range");
    GS_CHECK_ARG(c->focal_x > 0.f && c->focal_y > 0.f && std::isfinite(c->focal_x) && std::isfinite(c->focal_y),
                 "focal lengths must be positive and finite");
    return 0;
}

}  // namespace

extern "C" size_t gs_view_overlap_workspace_bytes(int32_t H, int32_t W, int32_t stride, int32_t n_views) {
    if (H <= 0 || W <= 0 || stride < 1 || n_views < 1 || n_views > GS_OVERLAP_MAX_VIEWS) return 0;
    const OverlapPlan P = overlap_plan(H, W, stride);
    return gs_align_up(sizeof(uint32_t) * (size_t)(P.nblk > 0 ? P.nblk : 1) * (size_t)(n_views + 2), 256);
}

extern "C" int gs_view_overlap_check_view(const gs_seed_camera *view, int32_t border) {
    int rc = overlap_check_camera(view, "view is null");
    if (rc) return rc;
    GS_CHECK_ARG(border >= 0, "border must not be negative");
    GS_CHECK_ARG(2 * (int64_t)border < view->width && 2 * (int64_t)border < view->height,
                 "the border leaves nothing of the view's image");
    return 0;
}

// gs_view_overlap (pp = nullptr) and gs_view_overlap_pp (pp = the frame's offsets, view_pp_dev = the views'; no offset anywhere
// runs gs_view_overlap's kernel)
static int gs_view_overlap_impl(const float *range, const gs_seed_camera *cam, const float *pp, const gs_seed_camera *views_dev,
                             const float *view_pp_dev, int32_t n_views, const gs_overlap_opts *opts, int64_t *counts_dev,
                             void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    int rc = overlap_check_opts(opts);
    if (rc) return rc;
    rc = overlap_check_camera(cam, "camera is null");
    if (rc) return rc;
    GS_CHECK_ARG(((uintptr_t)view_pp_dev & 7) == 0, "view_pp_dev must be 8-byte aligned");
    GS_CHECK_ARG(range != nullptr, "range is null");
    GS_CHECK_ARG(n_views >= 1 && n_views <= GS_OVERLAP_MAX_VIEWS, "n_views must lie in [1, GS_OVERLAP_MAX_VIEWS]");
    GS_CHECK_ARG(views_dev != nullptr, "views_dev is null");
    GS_CHECK_ARG(((uintptr_t)views_dev & 63) == 0, "views_dev must be 64-byte aligned");
    GS_CHECK_ARG(counts_dev != nullptr && ((uintptr_t)counts_dev & 7) == 0, "counts_dev null or misaligned");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0
                     && workspace_bytes >= gs_view_overlap_workspace_bytes(cam->height, cam->width, opts->stride, n_views),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const OverlapPlan P = overlap_plan(cam->height, cam->width, opts->stride);
    uint32_t *rows = (uint32_t *)workspace;
    const bool off_centre = (pp && (pp[0] != 0.f || pp[1] != 0.f)) || view_pp_dev;
    if (P.nblk > 0 && off_centre) {
        gs_seed_camera_pp c;
        c.cam = *cam;
        c.pp_dx = pp ? pp[0] : 0.f;
        c.pp_dy = pp ? pp[1] : 0.f;
        hipLaunchKernelGGL(overlap_count_pp_kernel, dim3(P.nblk), dim3(OVL_BLOCK), 0, s, range, P.G, c, views_dev,
                           (const float2 *)view_pp_dev, n_views, opts->near, opts->border, rows);
        GS_CHECK_LAUNCH();
    } else if (P.nblk > 0) {
        hipLaunchKernelGGL(overlap_count_kernel, dim3(P.nblk), dim3(OVL_BLOCK), 0, s, range, P.G, *cam, views_dev, n_views,
                           opts->near, opts->border, rows);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(overlap_finalize_kernel, dim3((n_views + 2 + 63) / 64), dim3(OVL_BLOCK), 0, s, rows, P.nblk, n_views + 2,
                       (long long *)counts_dev);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_view_overlap(const float *range, const gs_seed_camera *cam, const gs_seed_camera *views_dev,
                               int32_t n_views, const gs_overlap_opts *opts, int64_t *counts_dev, void *workspace,
                               size_t workspace_bytes, gs_stream_t stream) {
    return gs_view_overlap_impl(range, cam, nullptr, views_dev, nullptr, n_views, opts, counts_dev, workspace, workspace_bytes,
                             stream);
}

extern "C" int gs_view_overlap_pp(const float *range, const gs_seed_camera_pp *cam, const gs_seed_camera *views_dev,
                                  const float *view_pp_dev, int32_t n_views, const gs_overlap_opts *opts, int64_t *counts_dev,
                                  void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    GS_CHECK_ARG(cam != nullptr, "camera is null");
    GS_CHECK_ARG(std::isfinite(cam->pp_dx) && std::isfinite(cam->pp_dy), "the principal point's offset must be finite");
    const float pp[2] = {cam->pp_dx, cam->pp_dy};
    return gs_view_overlap_impl(range, &cam->cam, pp, views_dev, view_pp_dev, n_views, opts, counts_dev, workspace, workspace_bytes,
                             stream);
}
