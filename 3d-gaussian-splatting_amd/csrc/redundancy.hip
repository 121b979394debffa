// redundancy.hip -- how many OTHER views see each surface point one view measured (gs_view_redundancy, include/gs_abi.h).
//
// overlap.hip answers per view ("how many of the frame's points does view k see"); eviction of a keyframe asks per point:
// "this keyframe can go because nearly all it measured is seen by at least m others".  The points are overlap.hip's -- the
// measured pixels of the source view's `stride` lattice, back-projected by overlap_point.h -- and so is every decision;
// what differs is where the count is kept.  Two launches, no atomics:
//   R1 redundancy_count_kernel    : overlap_count_kernel's geometry -- a 256-thread workgroup takes a run of consecutive
//                                   lattice pixels 256 at a time, a thread per pixel, the world point in three registers,
//                                   the view loop uniform across the wave with the view's 64-byte row through uniform
//                                   (scalar) loads -- but each lane keeps ONE counter, c += seen: no ballot per view.  The
//                                   row k == self_index is skipped by the whole wave, and a wave leaves the loop once every
//                                   measured lane has c >= 7: the histogram cannot change any more.  At the end of a chunk
//                                   each bin b takes popcount(ballot(measured and min(c, 7) == b)) into a wave-uniform
//                                   register; the four waves meet in LDS (4 x 9 words) and the workgroup writes one row of
//                                   9 uint32.
//   R2 redundancy_finalize_kernel : one workgroup: thread t adds rows t, t + 256, ... in int64, nine columns each; a wave
//                                   adds its lanes by xor shuffles, the four sums meet in LDS and are added in wave order
//                                   -> hist_dev[9].  (Integer sums: the same number in any order.)
// Every row of the workspace that R2 reads was written whole by R1 in the same call: the result is a pure function of the
// inputs whatever the workspace and hist_dev held.  A wave none of whose 64 pixels carries a measurement skips the view loop.
// The launch plan is overlap.hip's, restated (the two are file-local; tests/test_redundancy_host.py holds this one against
// tests/overlap_ref.plan, which tests/test_overlap_host.py holds against overlap.hip's).
#include <cmath>

#include "gs_common.h"
#include "overlap_point.h"

namespace {

constexpr int RED_BLOCK = 256, RED_WAVES = RED_BLOCK / 64;
constexpr int RED_COLS = GS_REDUNDANCY_BINS + 1;  // the bins, then the measured lattice pixels
constexpr int RED_TOP = GS_REDUNDANCY_BINS - 1;   // the bin of "this many or more"
constexpr int RED_MAX_BLOCKS = 2048;              // 8 workgroups on each of 256 CUs: longer runs beyond that

struct RedundancyLattice {
    int32_t W, stride, off, Lw;  // pixel (lx * stride + off, ly * stride + off) for lattice index ly * Lw + lx
    int64_t L;                   // lattice pixels
    int32_t chunks_per_block;    // a workgroup's run: this many chunks of 256 lattice pixels
};

struct RedundancyPlan {
    RedundancyLattice G;
    int32_t nblk;  // workgroups of R1 = rows of the workspace
};

inline RedundancyPlan redundancy_plan(int32_t H, int32_t W, int32_t stride) {
    RedundancyPlan P;
    RedundancyLattice &G = P.G;
    G.W = W;
    G.stride = stride;
    G.off = stride / 2;
    G.Lw = W > G.off ? (W - G.off + stride - 1) / stride : 0;
    const int32_t Lh = H > G.off ? (H - G.off + stride - 1) / stride : 0;
    G.L = (int64_t)G.Lw * Lh;
    const int64_t chunks = gs_div_up(G.L, RED_BLOCK);
    G.chunks_per_block = (int32_t)(chunks > RED_MAX_BLOCKS ? gs_div_up(chunks, RED_MAX_BLOCKS) : 1);
    P.nblk = (int32_t)gs_div_up(chunks, G.chunks_per_block);
    return P;
}

// (one body, two kernels.  PP: the source camera and the views carry principal-point offsets -- the source's by value, view
// k's in row k of view_pp (nullptr: no view has one) -- and the *_pp decisions of overlap_point.h are taken.)
template <bool PP>
__device__ __forceinline__ void redundancy_count_body(const float *__restrict__ range, const RedundancyLattice &G,
                                                      const gs_seed_camera &cam, float cam_dx, float cam_dy,
                                                      const gs_seed_camera *__restrict__ views,
                                                      const float2 *__restrict__ view_pp, int32_t n_views,
                                                      int32_t self_index, float near, int32_t border,
                                                      uint32_t *__restrict__ rows) {
    __shared__ uint32_t s_hist[RED_WAVES][RED_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t hist[RED_COLS];  // (the same in every lane of the wave)
#pragma unroll
    for (int b = 0; b < RED_COLS; ++b) hist[b] = 0u;
    const int64_t chunk0 = (int64_t)blockIdx.x * G.chunks_per_block;
    for (int32_t ch = 0; ch < G.chunks_per_block; ++ch) {
        const int64_t base = (chunk0 + ch) * RED_BLOCK;
        if (base >= G.L) break;
        const int64_t j = base + threadIdx.x;
        bool meas = false;
        float p[3] = {0.f, 0.f, 0.f};
        if (j < G.L) {
            const int32_t ly = (int32_t)(j / G.Lw), lx = (int32_t)(j - (int64_t)ly * G.Lw);
            const int32_t x = lx * G.stride + G.off, y = ly * G.stride + G.off;
            const float z = range[(int64_t)y * G.W + x];
            meas = gs_overlap_measured(z);
            if (meas) {
                if (PP) gs_overlap_point_pp(cam, cam_dx, cam_dy, x, y, z, p);
                else gs_overlap_point(cam, x, y, z, p);
            }
        }
        const unsigned long long mm = __ballot(meas);
        if (mm == 0ull) continue;  // (the whole wave alike)
        int32_t c = 0;
        for (int k = 0; k < n_views; ++k) {
            if (k == self_index) continue;  // (uniform)
            bool seen;
            if (PP) {
                const float2 d = view_pp ? view_pp[k] : make_float2(0.f, 0.f);
                seen = gs_overlap_seen_pp(p, views[k], d.x, d.y, near, border);
            } else {
                seen = gs_overlap_seen(p, views[k], near, border);
            }
            c += seen ? 1 : 0;
            // every measured lane in the top bin: more views cannot change the histogram.  (Not free where no wave ever gets
            // there -- about a tenth of the loop's time, asked every view or every eighth alike)
            if (__ballot(meas && c < RED_TOP) == 0ull) break;
        }
        const int32_t bin = min(c, RED_TOP);
#pragma unroll
        for (int b = 0; b < GS_REDUNDANCY_BINS; ++b) hist[b] += (uint32_t)__popcll(__ballot(meas && bin == b));
        hist[GS_REDUNDANCY_BINS] += (uint32_t)__popcll(mm);
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < RED_COLS; ++b) s_hist[wave][b] = hist[b];
    }
    __syncthreads();
    if (threadIdx.x < RED_COLS) {
        const int b = threadIdx.x;
        rows[(size_t)blockIdx.x * RED_COLS + b] = s_hist[0][b] + s_hist[1][b] + s_hist[2][b] + s_hist[3][b];
    }
}

__global__ void __launch_bounds__(RED_BLOCK) redundancy_count_kernel(const float *__restrict__ range, RedundancyLattice G,
                                                                     gs_seed_camera cam,
                                                                     const gs_seed_camera *__restrict__ views,
                                                                     int32_t n_views, int32_t self_index, float near,
                                                                     int32_t border, uint32_t *__restrict__ rows) {
    redundancy_count_body<false>(range, G, cam, 0.f, 0.f, views, nullptr, n_views, self_index, near, border, rows);
}

__global__ void __launch_bounds__(RED_BLOCK) redundancy_count_pp_kernel(const float *__restrict__ range, RedundancyLattice G,
                                                                        gs_seed_camera_pp cam_pp,
                                                                        const gs_seed_camera *__restrict__ views,
                                                                        const float2 *__restrict__ view_pp, int32_t n_views,
                                                                        int32_t self_index, float near, int32_t border,
                                                                        uint32_t *__restrict__ rows) {
    redundancy_count_body<true>(range, G, cam_pp.cam, cam_pp.pp_dx, cam_pp.pp_dy, views, view_pp, n_views, self_index, near,
                                border, rows);
}

__global__ void __launch_bounds__(RED_BLOCK) redundancy_finalize_kernel(const uint32_t *__restrict__ rows, int32_t nblk,
                                                                        long long *__restrict__ hist) {
    __shared__ long long s_sum[RED_WAVES][RED_COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long sum[RED_COLS];
#pragma unroll
    for (int b = 0; b < RED_COLS; ++b) sum[b] = 0;
    for (int32_t r = threadIdx.x; r < nblk; r += RED_BLOCK) {
#pragma unroll
        for (int b = 0; b < RED_COLS; ++b) sum[b] += (long long)rows[(size_t)r * RED_COLS + b];
    }
#pragma unroll
    for (int b = 0; b < RED_COLS; ++b) {
        for (int off = 32; off > 0; off >>= 1) sum[b] += __shfl_xor(sum[b], off);
        if (lane == 0) s_sum[wave][b] = sum[b];
    }
    __syncthreads();
    if (threadIdx.x < RED_COLS) {
        const int b = threadIdx.x;
        hist[b] = s_sum[0][b] + s_sum[1][b] + s_sum[2][b] + s_sum[3][b];
    }
}

// (the argument checks of gs_view_overlap, restated: overlap.hip's are file-local)
int redundancy_check_opts(const gs_overlap_opts *o) {
    GS_CHECK_ARG(o != nullptr, "opts is null");
    GS_CHECK_ARG(o->stride >= 1, "stride must be >= 1");
    GS_CHECK_ARG(o->near > 0.f && std::isfinite(o->near), "near must be positive and finite");
    GS_CHECK_ARG(o->border >= 0, "border must not be negative");
    return 0;
}

int redundancy_check_camera(const gs_seed_camera *c) {
    GS_CHECK_ARG(c != nullptr, "camera is null");
    GS_CHECK_ARG(c->height > 0 && c->width > 0 && (int64_t)c->height * c->width < (1ll << 31), "image size out of range");
    GS_CHECK_ARG(c->focal_x > 0.f && c->focal_y > 0.f && std::isfinite(c->focal_x) && std::isfinite(c->focal_y),
                 "focal lengths must be positive and finite");
    return 0;
}

}  // namespace

extern "C" size_t gs_view_redundancy_workspace_bytes(int32_t H, int32_t W, int32_t stride) {
    if (H <= 0 || W <= 0 || stride < 1) return 0;
    const RedundancyPlan P = redundancy_plan(H, W, stride);
    return gs_align_up(sizeof(uint32_t) * (size_t)(P.nblk > 0 ? P.nblk : 1) * (size_t)RED_COLS, 256);
}

// gs_view_redundancy (pp = nullptr) and gs_view_redundancy_pp (pp = the source's offsets, view_pp_dev = the views'; no offset
// anywhere runs gs_view_redundancy's kernel)
static int gs_view_redundancy_impl(const float *range, const gs_seed_camera *cam, const float *pp,
                                   const gs_seed_camera *views_dev, const float *view_pp_dev, int32_t n_views,
                                   int32_t self_index, const gs_overlap_opts *opts, int64_t *hist_dev, void *workspace,
                                   size_t workspace_bytes, gs_stream_t stream) {
    int rc = redundancy_check_opts(opts);
    if (rc) return rc;
    rc = redundancy_check_camera(cam);
    if (rc) return rc;
    GS_CHECK_ARG(((uintptr_t)view_pp_dev & 7) == 0, "view_pp_dev must be 8-byte aligned");
    GS_CHECK_ARG(range != nullptr, "range is null");
    GS_CHECK_ARG(n_views >= 1 && n_views <= GS_OVERLAP_MAX_VIEWS, "n_views must lie in [1, GS_OVERLAP_MAX_VIEWS]");
    GS_CHECK_ARG(self_index >= -1 && self_index < n_views, "self_index must lie in [-1, n_views)");
    GS_CHECK_ARG(views_dev != nullptr, "views_dev is null");
    GS_CHECK_ARG(((uintptr_t)views_dev & 63) == 0, "views_dev must be 64-byte aligned");
    GS_CHECK_ARG(hist_dev != nullptr && ((uintptr_t)hist_dev & 7) == 0, "hist_dev null or misaligned");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0
                     && workspace_bytes >= gs_view_redundancy_workspace_bytes(cam->height, cam->width, opts->stride),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const RedundancyPlan P = redundancy_plan(cam->height, cam->width, opts->stride);
    uint32_t *rows = (uint32_t *)workspace;
    const bool off_centre = (pp && (pp[0] != 0.f || pp[1] != 0.f)) || view_pp_dev;
    if (P.nblk > 0 && off_centre) {
        gs_seed_camera_pp c;
        c.cam = *cam;
        c.pp_dx = pp ? pp[0] : 0.f;
        c.pp_dy = pp ? pp[1] : 0.f;
        hipLaunchKernelGGL(redundancy_count_pp_kernel, dim3(P.nblk), dim3(RED_BLOCK), 0, s, range, P.G, c, views_dev,
                           (const float2 *)view_pp_dev, n_views, self_index, opts->near, opts->border, rows);
        GS_CHECK_LAUNCH();
    } else if (P.nblk > 0) {
        hipLaunchKernelGGL(redundancy_count_kernel, dim3(P.nblk), dim3(RED_BLOCK), 0, s, range, P.G, *cam, views_dev, n_views,
                           self_index, opts->near, opts->border, rows);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(redundancy_finalize_kernel, dim3(1), dim3(RED_BLOCK), 0, s, rows, P.nblk, (long long *)hist_dev);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_view_redundancy(const float *range, const gs_seed_camera *cam, const gs_seed_camera *views_dev,
                                  int32_t n_views, int32_t self_index, const gs_overlap_opts *opts, int64_t *hist_dev,
                                  void *workspace, size_t workspace_bytes, gs_stream_t stream) {
    return gs_view_redundancy_impl(range, cam, nullptr, views_dev, nullptr, n_views, self_index, opts, hist_dev, workspace,
                                   workspace_bytes, stream);
}

extern "C" int gs_view_redundancy_pp(const float *range, const gs_seed_camera_pp *cam, const gs_seed_camera *views_dev,
                                     const float *view_pp_dev, int32_t n_views, int32_t self_index,
                                     const gs_overlap_opts *opts, int64_t *hist_dev, void *workspace, size_t workspace_bytes,
                                     gs_stream_t stream) {
    GS_CHECK_ARG(cam != nullptr, "camera is null");
    GS_CHECK_ARG(std::isfinite(cam->pp_dx) && std::isfinite(cam->pp_dy), "the principal point's offset must be finite");
    const float pp[2] = {cam->pp_dx, cam->pp_dy};
    return gs_view_redundancy_impl(range, &cam->cam, pp, views_dev, view_pp_dev, n_views, self_index, opts, hist_dev, workspace,
                                   workspace_bytes, stream);
}
