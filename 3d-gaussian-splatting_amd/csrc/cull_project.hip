// cull_project.hip -- frustum culling + 3D->2D EWA covariance projection, forward.
//
// Replaces global_culling_kernel (gaussian.cu:1182-1336), world2camera (:49-99) and jacobian (:10-47) of the reference,
// and provides the fused first stage of the frame path (gs_frame_forward): projection + activations + tile-rectangle
// count + per-block pair sums in ONE pass over the Gaussians, with the strip / table count and the occlusion-culled
// variant fused in (gs_stage_project).  The projection itself is project_common.h; its backward is project_bwd.hip.
//
// This file is compiled with -ffp-contract=off and evaluates every expression in the
// reference's source order, so that depth bits and tile rectangles (the integer inputs of the
// sort) are bit-identical to oracle/gs_oracle.c.  The stage is HBM-bound (40 B in, <=60 B out,
// ~300 flops per Gaussian); losing FMA contraction costs nothing measurable.
#include <atomic>
#include <mutex>

#include "gs_common.h"
#include "gs_frame_layout.h"
#include "project_common.h"
#include "strip_common.h"
#include "tile_bin_common.h"

namespace {

// ---------------------------------------------------------------- reference-API kernels
__global__ void __launch_bounds__(256) global_culling_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ rot, const float *__restrict__ tran, int64_t n, float near_plane,
    float half_w, float half_h, float *__restrict__ res_pos, float4 *__restrict__ res_cov,
    int64_t *__restrict__ mask) {
    Cam cam;
#pragma unroll
    for (int i = 0; i < 9; ++i) cam.rot[i] = rot[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cam.tran[i] = tran[i];
    for (int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < n;
         pid += (int64_t)gridDim.x * blockDim.x) {
        float p[3], s[3], pi[3], cv[4];
        load3(pos, pid, p);
        load3(scale, pid, s);
        float4 q4 = quat[pid];
        float q[4] = {q4.x, q4.y, q4.z, q4.w};
        if (!project(p, q, s, cam, near_plane, half_w, half_h, pi, cv)) continue;
        mask[pid] = 1;
        res_pos[pid * 3 + 0] = pi[0];
        res_pos[pid * 3 + 1] = pi[1];
        res_pos[pid * 3 + 2] = pi[2];
        res_cov[pid] = make_float4(cv[0], cv[1], cv[2], cv[3]);
    }
}

__global__ void __launch_bounds__(256) world2camera_kernel(const float *__restrict__ pos,
                                                          const float *__restrict__ rot,
                                                          const float *__restrict__ tran,
                                                          float *__restrict__ res, int64_t B) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        float p[3];
        load3(pos, i, p);
        res[i * 3 + 0] = p[0] * rot[0] + p[1] * rot[1] + p[2] * rot[2] + tran[0];
        res[i * 3 + 1] = p[0] * rot[3] + p[1] * rot[4] + p[2] * rot[5] + tran[1];
        res[i * 3 + 2] = p[0] * rot[6] + p[1] * rot[7] + p[2] * rot[8] + tran[2];
    }
}

__global__ void __launch_bounds__(256) world2camera_backward_kernel(const float *__restrict__ grad_out,
                                                                   const float *__restrict__ rot,
                                                                   float *__restrict__ grad_inp, int64_t B) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        float g[3];
        load3(grad_out, i, g);
        grad_inp[i * 3 + 0] = g[0] * rot[0] + g[1] * rot[3] + g[2] * rot[6];
        grad_inp[i * 3 + 1] = g[0] * rot[1] + g[1] * rot[4] + g[2] * rot[7];
        grad_inp[i * 3 + 2] = g[0] * rot[2] + g[1] * rot[5] + g[2] * rot[8];
    }
}

__global__ void __launch_bounds__(256) jacobian_kernel(const float *__restrict__ pos_cam,
                                                      float *__restrict__ jac, int64_t B) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        float u[3];
        load3(pos_cam, i, u);
        float *J = jac + i * 9;
        J[0] = 1 / u[2];
        J[1] = 0;
        J[2] = -u[0] / (u[2] * u[2]);
        J[3] = 0;
        J[4] = 1 / u[2];
        J[5] = -u[1] / (u[2] * u[2]);
        float rs = 1.0f / sqrtf(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
        J[6] = rs * u[0];
        J[7] = rs * u[1];
        J[8] = rs * u[2];
    }
}

// ---------------------------------------------------------------- fused frame stage S1
// One thread per Gaussian: activations -> project -> tile rectangle -> per-Gaussian record.
// Per-block sum of tiles_touched goes to block_sums[blockIdx.x] (input of the scan stage).
// (ProjectParams, the activations and make_params: project_common.h)

// "prob" (calc_tile_info_kernel2, gaussian.cu:138-195): tile i of an axis is listed unless
// `edge(i+1) < lo || hi < edge(i)`, with the tile edges of Tiles.create_tiles (splatter.py:275-293):
// edge(i) = (-pad/2 + 16 i) / focal, evaluated in fp32 exactly as torch does (an exact integer-valued float divided by
// the focal length; right(i) = left(i) + 16 before the division, so right(i) == left(i+1) bit for bit).  Both
// conditions are monotone in i, so the listed tiles are the range [first i with !(edge(i+1) < lo), last i with
// !(hi < edge(i))]: two binary searches with the reference's own comparisons (NaN bounds list every tile, as there).
__device__ __forceinline__ void edge_range(float lo, float hi, float half_pad, float focal, uint32_t n,
                                           uint32_t &i0, uint32_t &i1) {
    auto edge = [&](uint32_t i) { return (16.0f * (float)i - half_pad) / focal; };
    uint32_t a = 0, b = n;  // first i in [0, n] with !(edge(i+1) < lo)
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (edge(m + 1) < lo) a = m + 1; else b = m;
    }
    i0 = a;
    a = 0, b = n;  // first i in [0, n] with (hi < edge(i)): one past the last listed tile
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (hi < edge(m)) b = m; else a = m + 1;
    }
    i1 = a;
    if (i0 > i1) i0 = i1;
}

// Tile rectangle of calc_tile_info_kernel3 (gaussian.cu:226-242); count = 0 if det <= 0.
__device__ __forceinline__ uint32_t tile_rect(float cx, float cy, const float cv[4], const ProjectParams &P,
                                              uint32_t &y0, uint32_t &y1, uint32_t &x0, uint32_t &x1) {
    float det = (cv[0] * cv[3] - cv[1] * cv[2]);
    y0 = y1 = x0 = x1 = 0;
    if (det <= 0) return 0;
    float ai = (float)(cv[3] / (det + 1e-14));
    float di = (float)(cv[0] / (det + 1e-14));
    float shift_x = sqrtf(di * P.tlog * det);
    float shift_y = sqrtf(ai * P.tlog * det);
    float bbx_right = cx + shift_x, bbx_left = cx - shift_x;
    float bbx_top = cy - shift_y, bbx_bottom = cy + shift_y;
    if (P.cull_method == 1) {
        edge_range(bbx_left, bbx_right, P.half_padw, P.fx, P.ntx, x0, x1);
        edge_range(bbx_top, bbx_bottom, P.half_padh, P.fy, P.nty, y0, y1);
        return (y1 - y0) * (x1 - x0);
    }
    y0 = gs_f2u_sat(fmaxf((bbx_top - P.topmost) / P.tly, 0));
    y1 = gs_f2u_sat((bbx_bottom - P.topmost) / P.tly + 1);
    x0 = gs_f2u_sat(fmaxf((bbx_left - P.leftmost) / P.tlx, 0));
    x1 = gs_f2u_sat((bbx_right - P.leftmost) / P.tlx + 1);
    if (y1 > P.nty) y1 = P.nty;
    if (x1 > P.ntx) x1 = P.ntx;
    if (y0 > y1) y0 = y1;
    if (x0 > x1) x0 = x1;
    return (y1 - y0) * (x1 - x0);
}

// "dist" (calc_tile_info_kernel, gaussian.cu:101-136): a Gaussian is listed in every tile whose centre is closer than
// sqrt(thresh) to its own centre.  The listed tiles are decided per tile by gs_dist_listed (gs_common.h, the
// reference's own fp32 comparison); this is only the bounding square of the disc, with one tile of slack on every side
// (the index arithmetic below is not the reference's edge arithmetic; it is off by rounding only), over which the
// binning walks and the gradient rows are laid out.  NaN / infinite centres list nothing, as there.
__device__ __forceinline__ uint32_t dist_rect(float cx, float cy, const ProjectParams &P, uint32_t &y0, uint32_t &y1,
                                              uint32_t &x0, uint32_t &x1) {
    y0 = y1 = x0 = x1 = 0;
    if (!(fabsf(cx) < 3.0e38f) || !(fabsf(cy) < 3.0e38f) || !(P.dist_radius >= 0.f)) return 0;
    // tile centre i sits at (16 i + 8 - pad/2) / focal: i = ((c -+ r) focal + pad/2 - 8) / 16
    const float lx = ((cx - P.dist_radius) * P.fx + P.half_padw - 8.0f) * 0.0625f;
    const float hx = ((cx + P.dist_radius) * P.fx + P.half_padw - 8.0f) * 0.0625f;
    const float ly = ((cy - P.dist_radius) * P.fy + P.half_padh - 8.0f) * 0.0625f;
    const float hy = ((cy + P.dist_radius) * P.fy + P.half_padh - 8.0f) * 0.0625f;
    if (hx < -1.0f || hy < -1.0f || lx > (float)P.ntx || ly > (float)P.nty) return 0;
    // centres i with lx < i < hx can be listed: [ceil(lx), floor(hx)] -> one more on either side
    x0 = gs_f2u_sat(floorf(lx));
    y0 = gs_f2u_sat(floorf(ly));
    x1 = gs_f2u_sat(ceilf(hx) + 1.0f);
    y1 = gs_f2u_sat(ceilf(hy) + 1.0f);
    if (x1 > P.ntx) x1 = P.ntx;
    if (y1 > P.nty) y1 = P.nty;
    if (x0 > x1) x0 = x1;
    if (y0 > y1) y0 = y1;
    return (y1 - y0) * (x1 - x0);
}

// (RawGaussian, StaticGaussian and make_static: project_common.h)
__device__ __forceinline__ RawGaussian load_raw(const float *__restrict__ pos, const float4 *__restrict__ quat,
                                                const float *__restrict__ scale, const float *__restrict__ opa,
                                                const float *__restrict__ rgb, int64_t pid, int color_dim) {
    RawGaussian r;
    load3(pos, pid, r.p);
    load3(scale, pid, r.sraw);
    const float4 q4 = quat[pid];
    r.qraw[0] = q4.x; r.qraw[1] = q4.y; r.qraw[2] = q4.z; r.qraw[3] = q4.w;
    r.opa = opa[pid];
    r.rgb[0] = r.rgb[1] = r.rgb[2] = 0.f;
    if (color_dim == 3) load3(rgb, pid, r.rgb);
    return r;
}

// The raw parameters of the FIRST round are waited for before the loop is entered.  Without this the loop header merges
// "the prologue's loads are in flight" with the back edge's clean state, and the waitcnt pass, conservative across the
// merge, puts an `s_waitcnt vmcnt(1)` in front of the first use of the current round's quaternion -- right behind the
// five loads of the NEXT round, which are thereby waited for as well: the prefetch hid nothing.
__device__ __forceinline__ void settle(const RawGaussian &r) {
    asm volatile("" ::"v"(r.p[0]), "v"(r.p[1]), "v"(r.p[2]), "v"(r.sraw[0]), "v"(r.sraw[1]), "v"(r.sraw[2]), "v"(r.qraw[0]),
                 "v"(r.qraw[1]), "v"(r.qraw[2]), "v"(r.qraw[3]), "v"(r.opa), "v"(r.rgb[0]), "v"(r.rgb[1]), "v"(r.rgb[2]));
}

__device__ __forceinline__ void settle(const StaticGaussian &g) {
    asm volatile("" ::"v"(g.p[0]), "v"(g.p[1]), "v"(g.p[2]), "v"(g.opa_act), "v"(g.RSSR[0]), "v"(g.RSSR[1]), "v"(g.RSSR[2]),
                 "v"(g.RSSR[3]), "v"(g.RSSR[4]), "v"(g.RSSR[5]), "v"(g.RSSR[6]), "v"(g.RSSR[7]), "v"(g.RSSR[8]), "v"(g.col[0]),
                 "v"(g.col[1]), "v"(g.col[2]));
}

// The scene pack (include/gs_abi.h, GS_FRAME_SCENE_PACK): the camera-independent half of every Gaussian, computed once by
// scene_pack_build_kernel and read by the PACKED project kernels of the inference frames that follow.  Plane B, one aligned
// 64-byte record per Gaussian: {p.xyz, sigmoid(opa)} {RSSR[0..3]} {RSSR[4..7]} {RSSR[8], col.rgb}; plane A, a float4 per
// Gaussian: {p.xyz, smax}, what phase A of the occlusion-culled kernel streams.
__device__ __forceinline__ StaticGaussian load_static(const float4 *__restrict__ pack_b, int64_t pid) {
    const float4 *rec = pack_b + pid * 4;
    const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    StaticGaussian g;
    g.p[0] = a.x; g.p[1] = a.y; g.p[2] = a.z; g.opa_act = a.w;
    g.RSSR[0] = b.x; g.RSSR[1] = b.y; g.RSSR[2] = b.z; g.RSSR[3] = b.w;
    g.RSSR[4] = c.x; g.RSSR[5] = c.y; g.RSSR[6] = c.z; g.RSSR[7] = c.w;
    g.RSSR[8] = d.x; g.col[0] = d.y; g.col[1] = d.z; g.col[2] = d.w;
    return g;
}
__device__ __forceinline__ void store_static(float4 *__restrict__ pack_b, int64_t pid, const StaticGaussian &g) {
    float4 *rec = pack_b + pid * 4;
    rec[0] = make_float4(g.p[0], g.p[1], g.p[2], g.opa_act);
    rec[1] = make_float4(g.RSSR[0], g.RSSR[1], g.RSSR[2], g.RSSR[3]);
    rec[2] = make_float4(g.RSSR[4], g.RSSR[5], g.RSSR[6], g.RSSR[7]);
    rec[3] = make_float4(g.RSSR[8], g.col[0], g.col[1], g.col[2]);
}

// S1 for one Gaussian, camera half: project -> tile rectangle -> 64-byte record (visible Gaussians only) + the
// 16-byte rectangle record (every Gaussian).  Returns the rectangle record; `vis` = passed the frustum test; `cxy` = the
// projected centre (the "dist" listing test of the binning needs it).
// PP: the frame carries an off-centre principal point (project_common.h, project_cull<PP>)
template <bool PP = false>
__device__ __forceinline__ uint4 project_one(const StaticGaussian &in, int64_t pid, const ProjectParams &P,
                                             float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched,
                                             uint4 *__restrict__ rects, uint32_t &vis, float2 &cxy) {
    float pc[3], pi[3], cv[4];
    uint32_t cnt = 0;
    vis = 0;
    cxy = make_float2(0.f, 0.f);
    uint2 rc = make_uint2(0, 0);
    float depth = 0.f;
    // A culled Gaussian leaves 16 (20) bytes -- its all-zero rectangle, which is what every later stage looks at first
    // (rects[i].z, the depth bits, is 0 exactly for culled Gaussians: visible ones lie beyond the near plane) --
    // and NOT its 64-byte record: nothing reads the record of a Gaussian that is in no tile's list (21 % of the
    // Gaussians of the 2.4 M scene: 33 of this stage's 337 MB).  The record of a culled Gaussian is unspecified.
    if (project_cull<PP>(in.p, P, pc, pi)) {
        project_cov_static(pc, in.RSSR, P.cam, pi, cv);
        vis = 1;
        uint32_t y0, y1, x0, x1;
        cnt = P.cull_method == 0 ? dist_rect(pi[0], pi[1], P, y0, y1, x0, x1)
                                 : tile_rect(pi[0], pi[1], cv, P, y0, y1, x0, x1);
        rc = make_uint2(y0 | (y1 << 16), x0 | (x1 << 16));
        depth = pi[2];
        cxy = make_float2(pi[0], pi[1]);
        const float4 col = make_float4(in.col[0], in.col[1], in.col[2], 0.0f);
        float cA = 0.f, cB = 0.f, cC = 0.f;
        gs_conic(cv[0], cv[1], cv[2], cv[3], cA, cB, cC);
        float4 *rec = rec_geom + pid * GS_REC_STRIDE;  // one 64-byte record per Gaussian
        rec[0] = make_float4(pi[0], pi[1], pi[2], in.opa_act);
        rec[1] = make_float4(cv[0], cv[1], cv[2], cv[3]);
        rec[2] = col;
        rec[3] = make_float4(cA, cB, cC, 0.f);
    }
    if (tiles_touched) tiles_touched[pid] = cnt;  // read by the radix paths (sort_modes 0 / 1) only
    const uint4 out = make_uint4(rc.x, rc.y, __float_as_uint(depth), cnt);
    rects[pid] = out;
    return out;
}
// S1 from the raw parameters: load_raw -> make_static (activations, R S S R^T) -> the camera half
template <bool PP = false>
__device__ __forceinline__ uint4 project_one(const RawGaussian &in, int64_t pid, const ProjectParams &P,
                                             float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched,
                                             uint4 *__restrict__ rects, uint32_t &vis, float2 &cxy) {
    return project_one<PP>(make_static(in, P.scale_act, P.color_dim), pid, P, rec_geom, tiles_touched, rects, vis, cxy);
}

// One Gaussian per thread, grid-stride: both planes of the scene pack from the raw parameters (a stream: 56 B in, 80 B out).
// smax = the largest activated scale, NaN unless all three are finite (s0 + s1 + s2 < 3e38 as phase A of the raw kernel asks):
// the packed kernel's guard is then `smax < 3e38`, and a Gaussian with a non-finite scale is projected as it is there.
__global__ void __launch_bounds__(256) scene_pack_build_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, int scale_act, int color_dim,
    float4 *__restrict__ pack_a, float4 *__restrict__ pack_b) {
    for (int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < n; pid += (int64_t)gridDim.x * blockDim.x) {
        float s[3];
        const StaticGaussian g = make_static(load_raw(pos, quat, scale, opa, rgb, pid, color_dim), scale_act, color_dim, s);
        float smax = fmaxf(s[0], fmaxf(s[1], s[2]));
        if (!(s[0] + s[1] + s[2] < 3.0e38f)) smax = __uint_as_float(0x7fc00000u);
        pack_a[pid] = make_float4(g.p[0], g.p[1], g.p[2], smax);
        store_static(pack_b, pid, g);
    }
}

// (one body, two kernels, here and below: the kernel of a centred frame keeps its name, signature and code; *_pp_kernel is the
// instantiation for frames with an off-centre principal point, GS_FRAME_PRINCIPAL_POINT)
template <bool PP>
__device__ __forceinline__ void project_body(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, const ProjectParams &P,
    float4 *__restrict__ rec_geom,
    uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, uint32_t *__restrict__ block_sums,
    uint32_t *__restrict__ block_vis) {
    const int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t cnt = 0, vis = 0;
    if (pid < n) {
        float2 cxy;
        cnt = project_one<PP>(load_raw(pos, quat, scale, opa, rgb, pid, P.color_dim), pid, P, rec_geom, tiles_touched, rects,
                          vis, cxy).w;
    }
    // block sums of cnt and of the visible flag -> two plain stores per block (a same-address
    // atomic per block would serialise at ~12 ns each: 112 us for 2.4 M Gaussians)
    __shared__ uint32_t s_cnt[4], s_vis[4];
    uint32_t wsum = gs_wave_sum_u32(cnt), wvis = gs_wave_sum_u32(vis);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[wave] = wsum;
        s_vis[wave] = wvis;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        block_vis[blockIdx.x] = s_vis[0] + s_vis[1] + s_vis[2] + s_vis[3];
    }
}
__global__ void __launch_bounds__(256) frame_project_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom,
    uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, uint32_t *__restrict__ block_sums,
    uint32_t *__restrict__ block_vis) {
    project_body<false>(pos, quat, scale, opa, rgb, n, P, rec_geom, tiles_touched, rects, block_sums, block_vis);
}
__global__ void __launch_bounds__(256) frame_project_pp_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom,
    uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, uint32_t *__restrict__ block_sums,
    uint32_t *__restrict__ block_vis) {
    project_body<true>(pos, quat, scale, opa, rgb, n, P, rec_geom, tiles_touched, rects, block_sums, block_vis);
}

// ---------------------------------------------------------------- S1 + L1a fused (strip variant of sort_mode 2)
// Until round 3 frame_project_kernel wrote a 16-byte rectangle per Gaussian and a count kernel of strip_bin.hip read all
// of them back to histogram the strip entries: 38 MB and a 16-us launch at 2.4 M Gaussians for information that was in
// registers.  Here ONE workgroup per slice of the Gaussian array (the slices of the level-1 kernels: <= 256, dealt to
// the XCDs in contiguous runs) projects its Gaussians, 1024 at a time, and counts their strip entries on the spot -- one
// 64-bit LDS atomic per entry.  The raw parameters of the NEXT round are requested before the current one is projected
// (16 waves per CU hide the rest).  Outputs: records, rectangles, the [S][NS] table row of (entries << 32 | pairs) per
// strip, the slice's pair / visible counts; the one extra workgroup of the launch writes the tile dispatch order.
// Measured and dropped (round 3, same-box A/B): a COMPACTING variant of this kernel -- every wave tests 64 Gaussians
// against the frustum (~40 instructions), queues the survivors' raw parameters in a 128-entry LDS ring and runs the
// long half (~750 instructions) on full waves of survivors only, so that the 21 % culled Gaussians of the 2.4 M scene
// stop paying for it lane-masked.  Bit-identical outputs, 21 % fewer long-half wave passes -- and 89 - 92 us against
// 81 - 82 us for the kernel below (parameters loaded by index in the long half instead of queued: 93 us).
// PACKED: the frame carries a scene pack -- the kernel streams plane B (64 B per Gaussian in one aligned line, instead of 56 B
// from five arrays) and runs the camera half alone.
// (One body, two kernels: frame_project_count_kernel<DIST> reads the raw arrays and keeps its name and signature,
// frame_packed_project_count_kernel<DIST> is the PACKED instantiation.)
template <bool DIST, bool PACKED, bool PP>
__device__ __forceinline__ void project_count_body(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    extern __shared__ unsigned long long s_hist[];  // [NS] entries << 32 | pairs of this slice
    __shared__ uint32_t s_acc[2];
    // `gate`: the second, unculled pass of a GS_FRAME_OCCLUSION_CULL frame -- nothing to do unless a tile ran past its cut
    if (gate && *gate == 0) return;
    if (blockIdx.x >= S) {  // the one extra workgroup of the launch (uniform)
        tile_order_workgroup(tile_cost, n_tiles, tile_order);
        return;
    }
    // this launch covers the slices [slice0, slice0 + S): all of them, or one range of a frame whose project stage is
    // issued range by range (gs_frame_forward_project: the view-parallel trainer projects a range of Gaussians as soon
    // as their parameters have been updated)
    const uint32_t slice = slice0 + strip_slice_of_block(blockIdx.x, S);
    const int64_t g0 = (int64_t)slice * per_slice;
    auto in_range = [&](uint32_t i) { return i < per_slice && g0 + i < n; };
    auto load = [&](int64_t pid) {
        if constexpr (PACKED) return load_static(pack_b, pid);
        else return load_raw(pos, quat, scale, opa, rgb, pid, P.color_dim);
    };
    decltype(load(0)) cur = {}, nxt = {};
    if (in_range(threadIdx.x)) cur = load(g0 + threadIdx.x);
    for (uint32_t t = threadIdx.x; t < SG.NS; t += STRIP_THREADS) s_hist[t] = 0;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    settle(cur);
    uint32_t acc_cnt = 0, acc_vis = 0;
    for (uint32_t base = 0; base < per_slice; base += STRIP_THREADS) {  // uniform trip count
        const uint32_t i = base + threadIdx.x;
        if (in_range(i + STRIP_THREADS)) nxt = load(g0 + i + STRIP_THREADS);
        uint4 rc = make_uint4(0, 0, 0, 0);
        uint32_t vis = 0;
        float2 cxy = make_float2(0.f, 0.f);
        if (in_range(i)) rc = project_one<PP>(cur, g0 + i, P, rec_geom, tiles_touched, rects, vis, cxy);
        acc_cnt += rc.w;
        acc_vis += vis;
        walk_strips<DIST>(rc, g0 + i, SG, cxy, D,
                          [&](uint32_t strip, uint32_t, uint32_t, uint32_t np) { atomicAdd(&s_hist[strip], (1ull << 32) | np); });
        cur = nxt;
    }
    // rectangle areas (= gradient-row slots; == pairs unless DIST) and visible Gaussians of this slice
    acc_cnt = gs_wave_sum_u32(acc_cnt);
    acc_vis = gs_wave_sum_u32(acc_vis);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_acc[0], acc_cnt);
        atomicAdd(&s_acc[1], acc_vis);
    }
    __syncthreads();
    unsigned long long *row = table + (size_t)slice * SG.NS;
    for (uint32_t t = threadIdx.x; t < SG.NS; t += STRIP_THREADS) row[t] = s_hist[t];
    if (threadIdx.x == 0) {
        slice_pairs[slice] = s_acc[0];
        slice_vis[slice] = s_acc[1];
    }
}

template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_project_count_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    project_count_body<DIST, false, false>(pos, quat, scale, opa, rgb, nullptr, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                    tile_cost, n_tiles, tile_order, gate);
}
template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_packed_project_count_kernel(
    const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    project_count_body<DIST, true, false>(nullptr, nullptr, nullptr, nullptr, nullptr, pack_b, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                    tile_cost, n_tiles, tile_order, gate);
}
template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_project_count_pp_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    project_count_body<DIST, false, true>(pos, quat, scale, opa, rgb, nullptr, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                          tile_cost, n_tiles, tile_order, gate);
}
template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_packed_project_count_pp_kernel(
    const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    project_count_body<DIST, true, true>(nullptr, nullptr, nullptr, nullptr, nullptr, pack_b, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                         tile_cost, n_tiles, tile_order, gate);
}
// GS_FRAME_DEVICE_POSE: the twins of frame_project_count_kernel / _pp_kernel whose pose is the 12 floats `cam_dev` points to as
// they stand when the kernel runs (a uniform 48-byte load) instead of the descriptor's: P.cam is replaced, the body is the
// unchanged one.  Kernels of their own names: the others keep their code.
template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_project_count_dp_kernel(
    const Cam *__restrict__ cam_dev, const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    P.cam = *cam_dev;
    project_count_body<DIST, false, false>(pos, quat, scale, opa, rgb, nullptr, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                           tile_cost, n_tiles, tile_order, gate);
}
template <bool DIST>
__global__ void __launch_bounds__(STRIP_THREADS) frame_project_count_pp_dp_kernel(
    const Cam *__restrict__ cam_dev, const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint32_t *__restrict__ tiles_touched, uint4 *__restrict__ rects, GsDistCull D,
    uint32_t per_slice, gs_strip_geom SG, uint32_t S, uint32_t slice0, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis, const uint32_t *__restrict__ tile_cost,
    uint32_t n_tiles, uint32_t *__restrict__ tile_order, const unsigned long long *__restrict__ gate) {
    P.cam = *cam_dev;
    project_count_body<DIST, false, true>(pos, quat, scale, opa, rgb, nullptr, n, P, rec_geom, tiles_touched, rects, D, per_slice, SG, S, slice0, table, slice_pairs, slice_vis,
                                          tile_cost, n_tiles, tile_order, gate);
}

// ---------------------------------------------------------------- S1 + L1a of an occlusion-culled frame (first pass)
// GS_FRAME_OCCLUSION_CULL (gs_frame_layout.h): the previous frame of this workspace left, per tile, the depth behind which
// nothing was composited (`cut`).  74 % of the pairs of the opaque 2.4 M-Gaussian scene lie behind their tile's cut, and
// more than half of the visible Gaussians have NO pair in front of one -- yet every one of them paid the ~750 instructions
// of the projection.  Lane-masking them out gains nothing (a wave skips only what all of its 64 lanes skip, and Gaussians
// arrive in no spatial order: measured, 92.7 against 79 us), so this kernel COMPACTS:
//   phase A, every Gaussian of the slice: position and scale only (24 of 56 bytes), the exact frustum test, and a
//     conservative occlusion test (occluded_everywhere) -- ~120 instructions; the survivors' indices go to an LDS ring of
//     the wave that tested them;
//   phase B, full waves of survivors (a wave drains its ring whenever it holds 64: the two phases interleave, wave by
//     wave): the unchanged project_one + the trimmed strip walk of the culled frame, which counts
//     every level-1 entry and stores it, with its strip and its rank in the slice's run of that strip, in the slice's
//     staging region: the level-1 placement of this pass is a permutation of the staged entries (strip_bin.hip).
// A Gaussian that fails the occlusion test would have lost every pair to the trimming of walk_strips<.., true>: the
// emitted lists are exactly those of the lane-masked kernel, and the frame's second pass (a tile ran past its cut) starts
// from a gated re-run of frame_project_count_kernel, which rewrites records, rectangles and the strip table untrimmed.
// The cut pyramid: level 0 = the per-tile cuts (rows padded to whole strips, what walk_strips reads), level l = the LARGEST
// cut of each block of 2^l x 2^l tiles (GS_NO_CUT -- a tile that did not saturate -- is the largest value there is).
#define GS_OCC_LEVELS 4      // pyramid levels 0..3: rectangles of up to 16 x 16 tiles are tested with <= 3 x 3 look-ups
struct OccPyramid {
    const uint32_t *t0;           // level 0
    uint32_t o1, o2, o3;          // words from level l - 1's table to level l's
    uint32_t st0, d1, d2, d3;     // row stride of level 0; stride of level l minus stride of level l - 1 (mod 2^32)
};
// Is the Gaussian behind the cut of every tile its rectangle can reach?  Conservative by construction: the rectangle's
// half extents are sqrt(tlog S00) and sqrt(tlog S11) (tile_rect; its +1e-14 only shrinks them), S00 = r0 (R S S R^T) r0^T
// with r0 the first row of J W, so S00 <= s_max^2 |r0|^2 = s_max^2 (1 + (x/z)^2) / z^2 (W and R orthonormal: P.occ_k
// carries W's largest singular value, sqrt(tlog) and 2 % for the roundings -- fp32's are 1e-6), likewise S11; the tile
// range follows tile_rect's "prob2" arithmetic, monotone in the extents, with 1e-3 tile of slack.  Anything not finite,
// larger than 16 tiles, or another listing method: not tested (false).
template <bool PP>
__device__ __forceinline__ bool occluded_everywhere(const float pi[3], float z, float smax, uint32_t dbits,
                                                    const ProjectParams &P, const OccPyramid &Y) {
    if (P.cull_method != 2) return false;
    const float k = P.occ_k * smax * gs_rcp(z);
    // (GS_FRAME_PRINCIPAL_POINT: pi is the SHIFTED centre, which is what the tile arithmetic below wants; the bound on the
    // extent is a function of x / z itself, pi - s up to a rounding the 1.0001 covers)
    const float ux = PP ? pi[0] - P.sx : pi[0], uy = PP ? pi[1] - P.sy : pi[1];
    const float ax = 1.0f + ux * ux, ay = 1.0f + uy * uy;
    const float rx = k * (ax * gs_rsq(ax)) * 1.0001f, ry = k * (ay * gs_rsq(ay)) * 1.0001f;
    const float fx0 = (pi[0] - rx - P.leftmost) * P.inv_tlx - 1e-3f, fx1 = (pi[0] + rx - P.leftmost) * P.inv_tlx + 1e-3f;
    const float fy0 = (pi[1] - ry - P.topmost) * P.inv_tly - 1e-3f, fy1 = (pi[1] + ry - P.topmost) * P.inv_tly + 1e-3f;
    if (!(fx1 - fx0 < 16.0f) || !(fy1 - fy0 < 16.0f)) return false;  // large or not finite: projected
    // beside the grid (23 % of the Gaussians inside the frustum test of the 2.4 M scene: its margin is wider than the image):
    // tile_rect's range is empty -- x1 = floor(v + 1) = 0 for v < 0, x0 >= ntx >= x1 on the other side -- no tile, skipped
    if (fx1 < 0.f || fy1 < 0.f) return true;
    uint32_t x0 = gs_f2u_sat(fx0), y0 = gs_f2u_sat(fy0), x1 = gs_f2u_sat(fx1), y1 = gs_f2u_sat(fy1);  // tiles [x0, x1] x [y0, y1]
    if (x0 >= P.ntx || y0 >= P.nty) return true;
    x1 = x1 < P.ntx ? x1 : P.ntx - 1;
    y1 = y1 < P.nty ? y1 : P.nty - 1;
    const uint32_t e = (x1 - x0) > (y1 - y0) ? (x1 - x0) : (y1 - y0);
    const uint32_t L = e <= 1 ? 0u : (e <= 3 ? 1u : (e <= 7 ? 2u : 3u));  // (x1 >> L) - (x0 >> L) <= 2 then
    // (level L's table starts off[L] words behind level 0's; selected arithmetically: a select between the struct's fields
    // became a load from a scratch copy of it)
    const uint32_t m1 = L >= 1 ? ~0u : 0u, m2 = L >= 2 ? ~0u : 0u, m3 = L >= 3 ? ~0u : 0u;
    const uint32_t *tab = Y.t0 + ((Y.o1 & m1) + (Y.o2 & m2) + (Y.o3 & m3));
    const uint32_t st = Y.st0 + ((Y.d1 & m1) + (Y.d2 & m2) + (Y.d3 & m3));
    const uint32_t cx0 = x0 >> L, cy0 = y0 >> L, w = (x1 >> L) - cx0, h = (y1 >> L) - cy0;  // w, h in 0..2
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j)
#pragma unroll
        for (uint32_t i = 0; i < 3; ++i) {
            const uint32_t c = tab[(cy0 + (j < h ? j : h)) * st + cx0 + (i < w ? i : w)];
            m = c > m ? c : m;
        }
    return dbits > m;
}

// Measured and dropped (profiles/cull_waves_ab.txt): this kernel with ONE survivor queue per workgroup -- every wave of phase A
// claimed its slots with a returning LDS add on one word, a barrier, then phase B on the queue, 1,024 survivors at a time.
// All 16 waves of the CU's one workgroup streamed at the same moment and then all of them waited for the same sparse gather.
// Now every wave compacts for itself and projects its survivors as soon as it has 64 of them: no wave waits for another one
// before the end of the slice, and on a SIMD one wave's gather lies under the other waves' stream.
#define GS_OCC_RING 128u     // slots of a wave's survivor ring: a round adds at most 64, 64 are drained whenever 64 are present
#define GS_OCC_TAIL (16u * 63u)  // the leftovers of the 16 waves (fewer than 64 each), pooled at the end of the slice

// PACKED (the frame carries a scene pack): phase A streams plane A -- one 16-byte load per Gaussian, position and the largest
// activated scale, 38 MB instead of 58 and no exponential --, the drain gathers the survivor's one 64-byte line of plane B and
// runs the camera half alone.  The ring carries indices only: nothing phase A read is needed again.  Pyramid, strip walk,
// staging and every output are those of the raw variant.
// (One body, two kernels, as above: frame_project_cull_count_kernel and frame_packed_project_cull_count_kernel.)
template <bool PACKED, bool PP>
__device__ __forceinline__ void project_cull_count_body(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, const float4 *__restrict__ pack_a,
    const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, uint32_t per_slice, gs_strip_geom SG, uint32_t S,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis,
    const uint32_t *__restrict__ tile_cost, uint32_t n_tiles, uint32_t *__restrict__ tile_order,
    const uint32_t *__restrict__ cut, uint32_t par_slots, unsigned long long *__restrict__ stage_ent,
    uint32_t *__restrict__ stage_tag, uint32_t ecap, uint32_t *__restrict__ slice_entries) {
    extern __shared__ unsigned long long s_hist[];  // [NS] entries << 32 | pairs of this slice, then the pyramid, rings and tail
    __shared__ uint32_t s_acc[2], s_tn, s_ne;
    if (blockIdx.x >= S) {  // the one extra workgroup of the launch (uniform)
        tile_order_workgroup(tile_cost, n_tiles, tile_order);
        return;
    }
    const uint32_t slice = strip_slice_of_block(blockIdx.x, S);
    const int64_t g0 = (int64_t)slice * per_slice;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- LDS: histogram | cut pyramid | 16 survivor rings | pooled tail | (raw variant) the ring slots' positions and scales
    uint32_t *s_cut = reinterpret_cast<uint32_t *>(s_hist + SG.NS);
    const uint32_t st0 = SG.nsx * GS_STRIP_W;
    const uint32_t w1 = (SG.ntx + 1) / 2, h1 = (SG.nty + 1) / 2, w2 = (w1 + 1) / 2, h2 = (h1 + 1) / 2, w3 = (w2 + 1) / 2,
                   h3 = (h2 + 1) / 2;
    uint32_t *s_l1 = s_cut + st0 * SG.nty, *s_l2 = s_l1 + w1 * h1, *s_l3 = s_l2 + w2 * h2;
    uint32_t *s_tail = s_l3 + w3 * h3 + (STRIP_THREADS / 64) * GS_OCC_RING;
    uint32_t *const ring = s_l3 + w3 * h3 + wave * GS_OCC_RING;  // this wave's: slice-relative indices of its survivors
    // the first `par_slots` slots of every ring keep position and scale as well (six planes of par_slots floats per wave): the
    // drain then gathers only the 32 bytes phase A did not read -- 17 % of the array still touches 62 % of its 64-byte lines
    float *const par = reinterpret_cast<float *>(s_tail + GS_OCC_TAIL) + wave * 6 * par_slots;
    const OccPyramid Y = {s_cut, st0 * SG.nty, w1 * h1, w2 * h2, st0, w1 - st0, w2 - w1, w3 - w2};
    // the first two rounds of positions and scales are requested before the set-up (their latency runs underneath it)
    auto fetch = [&](float (&pp)[3], float (&ss)[3], uint32_t i) {
        int64_t g = g0 + i;
        g = g < n ? g : n - 1;
        if constexpr (PACKED) {  // (ss[0] = smax; ss[1], ss[2] are never read)
            const float4 v = pack_a[g];
            pp[0] = v.x; pp[1] = v.y; pp[2] = v.z; ss[0] = v.w;
            ss[1] = ss[2] = 0.f;
        } else {
            load3(pos, g, pp);
            load3(scale, g, ss);
        }
    };
    float pa[3], sa[3], pb[3], sb[3];
    fetch(pa, sa, threadIdx.x);
    fetch(pb, sb, threadIdx.x + STRIP_THREADS);
    for (uint32_t t = threadIdx.x; t < SG.NS; t += STRIP_THREADS) s_hist[t] = 0;
    // (eight loads of the cut table in flight per thread: one at a time, each waited for, was 8 x the latency of a load)
    for (uint32_t t0 = threadIdx.x; t0 < st0 * SG.nty; t0 += 8 * STRIP_THREADS) {
        uint32_t v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t t = t0 + k * STRIP_THREADS, iy = t / st0, ix = t - iy * st0;
            const bool in = iy < SG.nty && ix < SG.ntx;
            v[k] = cut[in ? iy * SG.ntx + ix : 0u];
            v[k] = in ? v[k] : GS_NO_CUT;
        }
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            if (t0 + k * STRIP_THREADS < st0 * SG.nty) s_cut[t0 + k * STRIP_THREADS] = v[k];
    }
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    if (threadIdx.x == 2) s_ne = 0;
    if (threadIdx.x == 3) s_tn = 0;
    // this slice's region of the entry staging (gs_frame_layout.h, gs_cull_stage_cap): `ecap` entries and their tags
    unsigned long long *const ent = stage_ent + (size_t)slice * ecap;
    uint32_t *const tag = stage_tag + (size_t)slice * ecap;
    auto build = [&](uint32_t *dst, uint32_t dw, uint32_t dh, const uint32_t *src, uint32_t sst, uint32_t sw, uint32_t sh) {
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < dw * dh; t += STRIP_THREADS) {
            const uint32_t cy = t / dw, cx = t - cy * dw, x = 2 * cx, y = 2 * cy;
            uint32_t m = src[y * sst + x];
            if (x + 1 < sw) m = max(m, src[y * sst + x + 1]);
            if (y + 1 < sh) {
                m = max(m, src[(y + 1) * sst + x]);
                if (x + 1 < sw) m = max(m, src[(y + 1) * sst + x + 1]);
            }
            dst[t] = m;
        }
    };
    build(s_l1, w1, h1, s_cut, st0, SG.ntx, SG.nty);
    build(s_l2, w2, h2, s_l1, w1, w1, h1);
    build(s_l3, w3, h3, s_l2, w2, w2, h2);
    __syncthreads();  // the pyramid is complete; from here to the pooled tail no wave waits for another one
    uint32_t acc_cnt = 0, acc_vis = 0;
    uint32_t head = 0, tail = 0;  // (wave-uniform) the ring holds the survivors [head, tail), slot = position mod GS_OCC_RING
    // the ring is written and read by this wave alone: LDS runs a wave's accesses in order, the compiler is told to keep them so
    auto ring_order = [] {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    // ---- the test of phase A: frustum + occlusion test of 64 Gaussians; the survivors go to the wave's ring
    // The phase is a stream (PACKED: 16 B in per Gaussian, nothing out) at one workgroup per CU: three rounds of positions and
    // scales are kept in flight.  That takes THREE NAMED register sets and a loop unrolled by three -- rotating one set into
    // the next at the end of a round (`cur = nxt`) makes the move wait for the newest load (first version: s_waitcnt vmcnt(0)
    // in every round, 30 us for the bare stream) -- and loads whose control flow is uniform (a lane beyond the slice loads the
    // array's last Gaussian and drops it), so that the waitcnt pass counts them exactly.
    auto in_slice = [&](uint32_t i) { return i < per_slice && g0 + i < n; };
    auto test = [&](const float (&pp)[3], const float (&ss)[3], uint32_t i) {
        bool surv = false;
        if (in_slice(i)) {
            float pc[3], pi[3];
            if (project_cull<PP>(pp, P, pc, pi)) {
                const float dep = sqrtf(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);  // == project_cov's pos_i[2]
                float smax;
                bool finite;
                if constexpr (PACKED) {  // (the pack holds NaN for a Gaussian whose scales are not all finite)
                    smax = ss[0];
                    finite = smax < 3.0e38f;
                } else {
                    float s[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) s[k] = P.scale_act == 0 ? fabsf(ss[k]) + 1e-4f : gs_exp2(GS_LOG2E * ss[k]);
                    smax = fmaxf(s[0], fmaxf(s[1], s[2]));
                    // (a NaN scale slips through fmaxf: s0 + s1 + s2 is NaN then, and the Gaussian is projected)
                    finite = s[0] + s[1] + s[2] < 3.0e38f;
                }
                if (finite && occluded_everywhere<PP>(pi, pc[2], smax, __float_as_uint(dep), P, Y)) {
                    // behind every cut it can reach, or beside the grid: visible, no tile.  NOTHING is written for it (nor
                    // for a Gaussian outside the frustum): this pass places the entries the drain stages, the second
                    // pass re-projects everything -- rects[] of a culled frame is only fresh for the survivors
                    acc_vis += 1;
                } else {
                    surv = true;
                }
            }
        }
        // no atomic, no shuffle: the wave's count is the ballot's population (an SGPR), a lane's slot the survivors below it
        const unsigned long long b = __ballot(surv);
        if (surv) {
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            const uint32_t slot = (tail + below) & (GS_OCC_RING - 1);
            ring[slot] = i;
            if (!PACKED && slot < par_slots) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    par[c * par_slots + slot] = pp[c];
                    par[(3 + c) * par_slots + slot] = ss[c];
                }
            }
        }
        tail += (uint32_t)__popcll(b);
    };
    // ---- the drain (phase B on this wave's own survivors): the unchanged project_one + the trimmed strip walk of the culled
    // frame, which counts every level-1 entry and stores it, with its strip and its rank in the slice's run of that strip, in
    // the slice's staging region
    // `slot`: the survivor's ring slot (raw variant: below par_slots its position and scale are in LDS; GS_OCC_RING: not queued
    // with them, gathered again)
    auto load_survivor = [&](uint32_t slot, uint32_t q) {
        const int64_t pid = g0 + q;
        if constexpr (PACKED) {
            return load_static(pack_b, pid);
        } else {
            RawGaussian r;
            if (slot < par_slots) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    r.p[c] = par[c * par_slots + slot];
                    r.sraw[c] = par[(3 + c) * par_slots + slot];
                }
            } else {
                load3(pos, pid, r.p);
                load3(scale, pid, r.sraw);
            }
            const float4 q4 = quat[pid];
            r.qraw[0] = q4.x; r.qraw[1] = q4.y; r.qraw[2] = q4.z; r.qraw[3] = q4.w;
            r.opa = opa[pid];
            r.rgb[0] = r.rgb[1] = r.rgb[2] = 0.f;
            if (P.color_dim == 3) load3(rgb, pid, r.rgb);
            return r;
        }
    };
    using Survivor = decltype(load_survivor(0, 0));
    auto project_walk = [&](const Survivor &g, uint32_t q, bool active) {
        uint4 rc = make_uint4(0, 0, 0, 0);
        uint32_t vis = 0;
        float2 cxy = make_float2(0.f, 0.f);
        const int64_t pid = g0 + q;
        if (active) rc = project_one<PP>(g, pid, P, rec_geom, nullptr, rects, vis, cxy);
        acc_cnt += rc.w;
        acc_vis += vis;
        // Every entry is counted AND kept: the LDS add returns the entry's rank inside this slice's run of its strip,
        // which with the column scan is its final position -- the permutation that follows (strip_bin.hip) neither walks
        // the rectangle nor reads the cut table again.  Slot in the slice's staging region: the lanes that arrive
        // together claim consecutive slots with one LDS add (they are whoever the walk has active here: the lowest of
        // them adds).  An entry beyond the region is not stored; the slice is withdrawn below.
        walk_strips<false, true>(rc, pid, SG, cxy, GsDistCull{},
                                 [&](uint32_t strip, uint32_t lo32, uint32_t d, uint32_t np) {
                                     const uint32_t rank = (uint32_t)(atomicAdd(&s_hist[strip], (1ull << 32) | np) >> 32);
                                     const unsigned long long act = __ballot(true);
                                     uint32_t wbase = 0;
                                     if ((int)lane == __ffsll((long long)act) - 1) wbase = atomicAdd(&s_ne, (uint32_t)__popcll(act));
                                     wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
                                     const uint32_t slot = wbase + (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
                                     if (slot < ecap) {
                                         ent[slot] = ((unsigned long long)d << 32) | lo32;
                                         tag[slot] = strip_tag(strip, rank);
                                     }
                                 },
                                 s_cut);
    };
    // A drain is cut in two: `request` takes the 64 oldest survivors off the ring and asks for their records, `finish` -- one
    // round of the test later, so that the gather's latency lies under it -- projects them (in one piece: 48.4 against 47.5 us
    // at 2.4 M Gaussians).  Both are wave-uniform branches: all 64 lanes are active in either.
    Survivor cur = {};
    uint32_t qi = 0;
    bool pending = false;  // (wave-uniform) `cur` / `qi` hold a requested, not yet projected survivor per lane
    auto request = [&] {
        if (tail - head >= 64u) {
            ring_order();
            const uint32_t slot = (head + lane) & (GS_OCC_RING - 1);
            qi = ring[slot];
            ring_order();  // (the next test's stores may reach these slots)
            head += 64u;
            cur = load_survivor(slot, qi);
            pending = true;
        }
    };
    auto finish = [&] {
        if (pending) {
            project_walk(cur, qi, true);
            pending = false;
        }
    };
    // The set the NEXT round tests is waited for before a drain's loads are requested behind it and before its stores go out:
    // where the two sides of a uniform branch meet, the waitcnt pass keeps the smaller count of "loads issued since", and the
    // wait for a set that was requested before the branch would take the gather (or the stores) with it.
    auto settle_set = [&](const float (&pp)[3], const float (&ss)[3]) {
        if constexpr (PACKED) asm volatile("" ::"v"(pp[0]), "v"(pp[1]), "v"(pp[2]), "v"(ss[0]));
        else asm volatile("" ::"v"(pp[0]), "v"(pp[1]), "v"(pp[2]), "v"(ss[0]), "v"(ss[1]), "v"(ss[2]));
    };
    float pq[3], sq[3];
    for (uint32_t base = 0; base < per_slice; base += 3 * STRIP_THREADS) {  // uniform trip count, uniform exits
        const uint32_t i = base + threadIdx.x;
        fetch(pq, sq, i + 2 * STRIP_THREADS);
        test(pa, sa, i);
        settle_set(pb, sb);
        finish();
        request();
        if (base + STRIP_THREADS >= per_slice) break;
        fetch(pa, sa, i + 3 * STRIP_THREADS);
        test(pb, sb, i + STRIP_THREADS);
        settle_set(pq, sq);
        finish();
        request();
        if (base + 2 * STRIP_THREADS >= per_slice) break;
        fetch(pb, sb, i + 4 * STRIP_THREADS);
        test(pq, sq, i + 2 * STRIP_THREADS);
        settle_set(pa, sa);
        finish();
        request();
    }
    finish();
    // ---- the pooled tail: every wave has fewer than 64 survivors left; they are pooled (one LDS add per wave) and projected
    // by the first waves as full waves, the last of them ragged.  Every wave of the workgroup arrives here, Gaussians or not.
    {
        const uint32_t left = tail - head;  // < 64
        uint32_t tbase = 0;
        if (left) {  // (uniform per wave)
            if (lane == 0) tbase = atomicAdd(&s_tn, left);
            tbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)tbase);
            ring_order();
            if (lane < left) s_tail[tbase + lane] = ring[(head + lane) & (GS_OCC_RING - 1)];
        }
    }
    __syncthreads();
    {
        const uint32_t nt = s_tn;
        if (wave * 64u < nt) {  // (uniform per wave)
            const uint32_t k = threadIdx.x;
            const bool active = k < nt;
            const uint32_t q = active ? s_tail[k] : 0u;
            Survivor g = {};
            if (active) g = load_survivor(GS_OCC_RING, q);
            project_walk(g, q, active);
        }
    }
    acc_cnt = gs_wave_sum_u32(acc_cnt);
    acc_vis = gs_wave_sum_u32(acc_vis);
    if (lane == 0) {
        atomicAdd(&s_acc[0], acc_cnt);
        atomicAdd(&s_acc[1], acc_vis);
    }
    __syncthreads();
    // A slice whose entries did not fit its staging region publishes NO entries (an empty table row: nothing downstream
    // of this pass reads a slot that was not written) and marks itself; the permutation raises counters[GS_CNT_RANPAST] for
    // it, and the gated second pass renders the frame from the full lists.
    const uint32_t ne = s_ne;
    const bool fits = ne <= ecap;
    unsigned long long *row = table + (size_t)slice * SG.NS;
    for (uint32_t t = threadIdx.x; t < SG.NS; t += STRIP_THREADS) row[t] = fits ? s_hist[t] : 0ull;
    if (threadIdx.x == 0) {
        slice_pairs[slice] = s_acc[0];
        slice_vis[slice] = s_acc[1];
        slice_entries[slice] = fits ? ne : GS_STAGE_OVER;
    }
}

__global__ void __launch_bounds__(STRIP_THREADS) frame_project_cull_count_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, uint32_t per_slice, gs_strip_geom SG, uint32_t S,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis,
    const uint32_t *__restrict__ tile_cost, uint32_t n_tiles, uint32_t *__restrict__ tile_order,
    const uint32_t *__restrict__ cut, uint32_t par_slots, unsigned long long *__restrict__ stage_ent,
    uint32_t *__restrict__ stage_tag, uint32_t ecap, uint32_t *__restrict__ slice_entries) {
    project_cull_count_body<false, false>(pos, quat, scale, opa, rgb, nullptr, nullptr, n, P, rec_geom, rects, per_slice, SG, S, table, slice_pairs, slice_vis, tile_cost, n_tiles, tile_order, cut,
                                   par_slots, stage_ent, stage_tag, ecap, slice_entries);
}
__global__ void __launch_bounds__(STRIP_THREADS) frame_packed_project_cull_count_kernel(
    const float4 *__restrict__ pack_a, const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, uint32_t per_slice, gs_strip_geom SG, uint32_t S,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis,
    const uint32_t *__restrict__ tile_cost, uint32_t n_tiles, uint32_t *__restrict__ tile_order,
    const uint32_t *__restrict__ cut, uint32_t par_slots, unsigned long long *__restrict__ stage_ent,
    uint32_t *__restrict__ stage_tag, uint32_t ecap, uint32_t *__restrict__ slice_entries) {
    project_cull_count_body<true, false>(nullptr, nullptr, nullptr, nullptr, nullptr, pack_a, pack_b, n, P, rec_geom, rects, per_slice, SG, S, table, slice_pairs, slice_vis, tile_cost, n_tiles, tile_order, cut,
                                   par_slots, stage_ent, stage_tag, ecap, slice_entries);
}
__global__ void __launch_bounds__(STRIP_THREADS) frame_project_cull_count_pp_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, uint32_t per_slice, gs_strip_geom SG, uint32_t S,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis,
    const uint32_t *__restrict__ tile_cost, uint32_t n_tiles, uint32_t *__restrict__ tile_order,
    const uint32_t *__restrict__ cut, uint32_t par_slots, unsigned long long *__restrict__ stage_ent,
    uint32_t *__restrict__ stage_tag, uint32_t ecap, uint32_t *__restrict__ slice_entries) {
    project_cull_count_body<false, true>(pos, quat, scale, opa, rgb, nullptr, nullptr, n, P, rec_geom, rects, per_slice, SG, S, table, slice_pairs, slice_vis, tile_cost, n_tiles, tile_order, cut,
                                         par_slots, stage_ent, stage_tag, ecap, slice_entries);
}
__global__ void __launch_bounds__(STRIP_THREADS) frame_packed_project_cull_count_pp_kernel(
    const float4 *__restrict__ pack_a, const float4 *__restrict__ pack_b, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, uint32_t per_slice, gs_strip_geom SG, uint32_t S,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis,
    const uint32_t *__restrict__ tile_cost, uint32_t n_tiles, uint32_t *__restrict__ tile_order,
    const uint32_t *__restrict__ cut, uint32_t par_slots, unsigned long long *__restrict__ stage_ent,
    uint32_t *__restrict__ stage_tag, uint32_t ecap, uint32_t *__restrict__ slice_entries) {
    project_cull_count_body<true, true>(nullptr, nullptr, nullptr, nullptr, nullptr, pack_a, pack_b, n, P, rec_geom, rects, per_slice, SG, S, table, slice_pairs, slice_vis, tile_cost, n_tiles, tile_order, cut,
                                        par_slots, stage_ent, stage_tag, ecap, slice_entries);
}

// ---------------------------------------------------------------- S1 + B1 fused (table variant of sort_mode 2: small scenes)
// The same fusion for the table variant, which small scenes take: a frame of 10,000 Gaussians is six dependent launches
// of ~7 us each, so the launch that re-reads the rectangles to histogram them per (slice, tile) is worth removing for
// its latency alone.  One workgroup per slice (tile_bin.hip's slices: a multiple of 256 Gaussians), one LDS counter per
// tile; same outputs as frame_project_kernel + bin_count_kernel.
template <bool DIST, bool PP>
__device__ __forceinline__ void project_bin_count_body(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, const ProjectParams &P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, const GsDistCull &D, uint32_t per_block, uint32_t T,
    uint32_t *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis) {
    extern __shared__ uint32_t s_tile_hist[];  // [T]
    __shared__ uint32_t s_acc[2];
    const uint32_t slice = slice_of_block(blockIdx.x, gridDim.x);
    const int64_t g0 = (int64_t)slice * per_block;
    auto in_range = [&](uint32_t i) { return i < per_block && g0 + i < n; };
    RawGaussian cur = {}, nxt = {};
    if (in_range(threadIdx.x)) cur = load_raw(pos, quat, scale, opa, rgb, g0 + threadIdx.x, P.color_dim);
    for (uint32_t t = threadIdx.x; t < T; t += BIN_THREADS) s_tile_hist[t] = 0;
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
    __syncthreads();
    settle(cur);
    uint32_t acc_cnt = 0, acc_vis = 0;
    for (uint32_t base = 0; base < per_block; base += BIN_THREADS) {  // uniform trip count
        const uint32_t i = base + threadIdx.x;
        if (in_range(i + BIN_THREADS)) nxt = load_raw(pos, quat, scale, opa, rgb, g0 + i + BIN_THREADS, P.color_dim);
        uint4 rc = make_uint4(0, 0, 0, 0);
        uint32_t vis = 0;
        float2 cxy = make_float2(0.f, 0.f);
        if (in_range(i)) rc = project_one<PP>(cur, g0 + i, P, rec_geom, nullptr, rects, vis, cxy);
        acc_cnt += rc.w;
        acc_vis += vis;
        walk_rect<DIST>(rc, g0 + i, P.ntx, cxy, D, [&](uint32_t tile, uint32_t, uint32_t) { atomicAdd(&s_tile_hist[tile], 1u); });
        cur = nxt;
    }
    acc_cnt = gs_wave_sum_u32(acc_cnt);
    acc_vis = gs_wave_sum_u32(acc_vis);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_acc[0], acc_cnt);
        atomicAdd(&s_acc[1], acc_vis);
    }
    __syncthreads();
    uint32_t *row = table + (size_t)slice * T;
    for (uint32_t t = threadIdx.x; t < T; t += BIN_THREADS) row[t] = s_tile_hist[t];
    if (threadIdx.x == 0) {
        slice_pairs[slice] = s_acc[0];
        slice_vis[slice] = s_acc[1];
    }
}
template <bool DIST>
__global__ void __launch_bounds__(BIN_THREADS) frame_project_bin_count_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, GsDistCull D, uint32_t per_block, uint32_t T,
    uint32_t *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis) {
    project_bin_count_body<DIST, false>(pos, quat, scale, opa, rgb, n, P, rec_geom, rects, D, per_block, T, table, slice_pairs, slice_vis);
}
template <bool DIST>
__global__ void __launch_bounds__(BIN_THREADS) frame_project_bin_count_pp_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, GsDistCull D, uint32_t per_block, uint32_t T,
    uint32_t *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis) {
    project_bin_count_body<DIST, true>(pos, quat, scale, opa, rgb, n, P, rec_geom, rects, D, per_block, T, table, slice_pairs, slice_vis);
}
// GS_FRAME_DEVICE_POSE: the table variant's twins (see frame_project_count_dp_kernel)
template <bool DIST>
__global__ void __launch_bounds__(BIN_THREADS) frame_project_bin_count_dp_kernel(
    const Cam *__restrict__ cam_dev, const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, GsDistCull D, uint32_t per_block, uint32_t T,
    uint32_t *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis) {
    P.cam = *cam_dev;
    project_bin_count_body<DIST, false>(pos, quat, scale, opa, rgb, n, P, rec_geom, rects, D, per_block, T, table, slice_pairs, slice_vis);
}
template <bool DIST>
__global__ void __launch_bounds__(BIN_THREADS) frame_project_bin_count_pp_dp_kernel(
    const Cam *__restrict__ cam_dev, const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ opa, const float *__restrict__ rgb, int64_t n, ProjectParams P,
    float4 *__restrict__ rec_geom, uint4 *__restrict__ rects, GsDistCull D, uint32_t per_block, uint32_t T,
    uint32_t *__restrict__ table, uint32_t *__restrict__ slice_pairs, uint32_t *__restrict__ slice_vis) {
    P.cam = *cam_dev;
    project_bin_count_body<DIST, true>(pos, quat, scale, opa, rgb, n, P, rec_geom, rects, D, per_block, T, table, slice_pairs, slice_vis);
}

}  // namespace

// ================================================================= C ABI (section A)
extern "C" int gs_world2camera(const float *pos, const float *rot, const float *tran, float *res, int64_t B,
                               gs_stream_t stream) {
    GS_CHECK_ARG(B >= 0, "B < 0");
    if (B == 0) return 0;
    GS_CHECK_ARG(pos && rot && tran && res, "null pointer");
    hipLaunchKernelGGL(world2camera_kernel, dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, pos, rot,
                       tran, res, B);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_world2camera_backward(const float *grad_out, const float *rot, float *grad_inp, int64_t B,
                                        gs_stream_t stream) {
    GS_CHECK_ARG(B >= 0, "B < 0");
    if (B == 0) return 0;
    GS_CHECK_ARG(grad_out && rot && grad_inp, "null pointer");
    hipLaunchKernelGGL(world2camera_backward_kernel, dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream,
                       grad_out, rot, grad_inp, B);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_jacobian(const float *pos_cam, float *jac, int64_t B, gs_stream_t stream) {
    GS_CHECK_ARG(B >= 0, "B < 0");
    if (B == 0) return 0;
    GS_CHECK_ARG(pos_cam && jac, "null pointer");
    hipLaunchKernelGGL(jacobian_kernel, dim3(grid_for(B, 256)), dim3(256), 0, (hipStream_t)stream, pos_cam, jac, B);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_global_culling(const float *pos, const float *quat, const float *scale, const float *rot,
                                 const float *tran, int64_t N, float near_plane, float half_width,
                                 float half_height, float *res_pos, float *res_cov, int64_t *culling_mask,
                                 gs_stream_t stream) {
    GS_CHECK_ARG(N >= 0, "N < 0");
    if (N == 0) return 0;
    GS_CHECK_ARG(pos && quat && scale && rot && tran && res_pos && res_cov && culling_mask, "null pointer");
    GS_CHECK_ARG(((uintptr_t)quat & 15) == 0 && ((uintptr_t)res_cov & 15) == 0, "quat/res_cov must be 16-byte aligned");
    hipLaunchKernelGGL(global_culling_kernel, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pos,
                       (const float4 *)quat, scale, rot, tran, N, near_plane, half_width, half_height, res_pos,
                       (float4 *)res_cov, culling_mask);
    GS_CHECK_LAUNCH();
    return 0;
}

// ================================================================= scene pack
extern "C" size_t gs_scene_pack_bytes(int64_t N, size_t *a_bytes, size_t *b_bytes) {
    // 16 N and 64 N bytes, each rounded up to whole 256-byte units
    const size_t a = N < 0 ? 0 : ((size_t)N * 16 + 255) / 256 * 256, b = N < 0 ? 0 : ((size_t)N * 64 + 255) / 256 * 256;
    if (a_bytes) *a_bytes = a;
    if (b_bytes) *b_bytes = b;
    return a + b;
}

extern "C" int gs_scene_pack_build(const float *pos, const float *quat, const float *scale, const float *opa, const float *rgb,
                                   int64_t N, int32_t color_dim, int32_t scale_activation, void *pack_a, void *pack_b,
                                   gs_stream_t stream) {
    GS_CHECK_ARG(N >= 0 && N < (1ll << 31), "N out of range");
    GS_CHECK_ARG(color_dim == 3 || color_dim == 27 || color_dim == 48, "color_dim must be 3, 27 or 48");
    GS_CHECK_ARG(scale_activation == 0 || scale_activation == 1, "scale_activation must be 0 (abs) or 1 (exp)");
    if (N == 0) return 0;
    GS_CHECK_ARG(pos && quat && scale && opa && rgb && pack_a && pack_b, "null pointer");
    GS_CHECK_ARG(((uintptr_t)quat & 15) == 0, "quat must be 16-byte aligned");
    GS_CHECK_ARG(((uintptr_t)pack_a & 15) == 0 && ((uintptr_t)pack_b & 63) == 0,
                 "pack_a must be 16-byte aligned, pack_b 64-byte aligned");
    hipLaunchKernelGGL(scene_pack_build_kernel, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pos,
                       (const float4 *)quat, scale, opa, rgb, N, (int)scale_activation, (int)color_dim, (float4 *)pack_a,
                       (float4 *)pack_b);
    GS_CHECK_LAUNCH();
    return 0;
}

// ================================================================= frame stages (internal)
// slice_begin / slice_end: the slices of the Gaussian array to project (strip variant only: gs_frame_project_slices;
// every other path projects everything at once: 0, -1)
// `second_pass`: the unculled re-run of a GS_FRAME_OCCLUSION_CULL frame's project stage, gated on counters[GS_CNT_RANPAST]
int gs_stage_project(const gs_frame *f, const gs_frame_ws &ws, hipStream_t stream, int slice_begin, int slice_end,
                     bool second_pass) {
    ProjectParams P = make_params(f);
    // sort_modes 0 / 1 read tiles_touched (emit_pairs_kernel); sort_mode 2 reads the rectangle records only
    uint32_t *touched = f->sort_mode == 2 && gs_frame_geometry(f).n_tiles <= GS_BIN_MAX_TILES ? nullptr : ws.tiles_touched;
    if (gs_frame_uses_strips(f)) {  // project + strip count in one kernel
        touched = nullptr;
        gs_frame_geom G = gs_frame_geometry(f);
        const gs_strip_plan plan = gs_strip_plan_for(f->N, G.ntx, G.nty);
        const gs_strip_geom SG = plan.geom;
        const GsDistCull D = gs_frame_dist_cull(f);
        static std::mutex attr_mu;
        static std::atomic<uint64_t> attr_done{0};
        int dev = 0;
        GS_HIP(hipGetDevice(&dev));
        if (dev < 64 && !((attr_done.load(std::memory_order_acquire) >> dev) & 1)) {
            std::lock_guard<std::mutex> lock(attr_mu);
            for (const void *fn : {(const void *)frame_project_count_kernel<false>, (const void *)frame_project_count_kernel<true>,
                                   (const void *)frame_packed_project_count_kernel<false>, (const void *)frame_packed_project_count_kernel<true>,
                                   (const void *)frame_project_cull_count_kernel, (const void *)frame_packed_project_cull_count_kernel,
                                   (const void *)frame_project_count_pp_kernel<false>, (const void *)frame_project_count_pp_kernel<true>,
                                   (const void *)frame_packed_project_count_pp_kernel<false>,
                                   (const void *)frame_packed_project_count_pp_kernel<true>,
                                   (const void *)frame_project_cull_count_pp_kernel,
                                   (const void *)frame_packed_project_cull_count_pp_kernel,
                                   (const void *)frame_project_count_dp_kernel<false>, (const void *)frame_project_count_dp_kernel<true>,
                                   (const void *)frame_project_count_pp_dp_kernel<false>,
                                   (const void *)frame_project_count_pp_dp_kernel<true>})
                // (the kernels also hold ~17 KiB of static LDS -- the tile-order workgroup's bins --: the strip histogram, and the
                // cut pyramid + survivor queue behind it in a culled frame, get what gs_frame_occlusion_cull's room rule allows)
                GS_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, GS_BIN_LDS_BYTES - 8 * 4096));
            attr_done.fetch_or(1ull << dev, std::memory_order_release);
        }
        unsigned long long *table = (unsigned long long *)ws.strip_table;
        if (slice_end < 0) slice_end = (int)plan.slices;
        GS_CHECK_ARG(slice_begin >= 0 && slice_begin < slice_end && slice_end <= (int)plan.slices, "bad slice range");
        const uint32_t nsl = (uint32_t)(slice_end - slice_begin);
        // GS_FRAME_SCENE_PACK: the PACKED kernels read the caller's two planes (validated in gs_frame.hip) instead of the raw arrays
        const bool packed = gs_frame_scene_pack(f);
        const float4 *pack_a = packed ? (const float4 *)gs_frame_scene_fields(f)->scene_pack_a : nullptr;
        const float4 *pack_b = packed ? (const float4 *)gs_frame_scene_fields(f)->scene_pack_b : nullptr;
        // GS_FRAME_DEVICE_POSE (a training frame without a pack or a cull: gs_frame.hip, validate): the *_dp_kernel twins
        const Cam *cam_dev = (const Cam *)gs_frame_pose_dev(f);
        if (gs_frame_occlusion_cull(f) && !second_pass) {
            // GS_FRAME_OCCLUSION_CULL, first pass: Gaussians behind every cut they can reach are not projected, the level-1
            // entries of the others are trimmed by the cut table the previous frame of this workspace left
            GS_CHECK_ARG(slice_begin == 0 && nsl == plan.slices, "an occlusion-culled frame is projected in one piece");
            // LDS behind the strip histogram: the cut pyramid, the 16 waves' survivor rings, the pooled tail -- 12 KiB where the
            // workgroup-wide 16-bit queue took up to 32 KiB: gs_frame_occlusion_cull's room rule, which still reserves that, holds
            size_t lds = sizeof(unsigned long long) * SG.NS + gs_cull_pyramid_bytes(G.ntx, G.nty) +
                         sizeof(uint32_t) * ((STRIP_THREADS / 64) * GS_OCC_RING + GS_OCC_TAIL);
            // raw variant: what is left of the kernel's LDS room holds position and scale (24 B) of the first slots of every ring
            const size_t room = (size_t)GS_BIN_LDS_BYTES - 8 * 4096;
            uint32_t par_slots = room > lds ? (uint32_t)((room - lds) / (24 * (STRIP_THREADS / 64))) : 0u;
            if (par_slots > GS_OCC_RING) par_slots = GS_OCC_RING;
            if (packed) par_slots = 0;  // (the packed variant queues indices only; GS_OCC_STASH is ignored)
            // GS_OCC_STASH, read per frame: fewer parameter slots in the workgroup's rings (a sixteenth of the value per wave) --
            // the parity tests walk the gathered-again path with it.  GS_OCC_QCAP chunked the 16-bit queue this kernel no longer
            // has: still accepted, without effect.
            if (const char *e = getenv("GS_OCC_STASH")) {
                const long v = atol(e);
                if (v >= 0 && (uint32_t)(v / (STRIP_THREADS / 64)) < par_slots) par_slots = (uint32_t)(v / (STRIP_THREADS / 64));
            }
            lds += (size_t)par_slots * 24 * (STRIP_THREADS / 64);
#define GS_CULL_TAIL                                                                                                   \
    f->N, P, ws.rec_geom, ws.rects, plan.per_slice, SG, nsl, table, ws.slice_pairs, ws.slice_vis, ws.tile_cost,        \
        (uint32_t)G.n_tiles, ws.tile_order, gs_frame_cut_table(f, ws), par_slots, (unsigned long long *)ws.keys_b,       \
        ws.vals_b, gs_cull_stage_cap(f->max_pairs, plan.slices), ws.slice_entries
            if (packed && P.pp)
                hipLaunchKernelGGL(frame_packed_project_cull_count_pp_kernel, dim3(nsl + 1), dim3(STRIP_THREADS), lds, stream,
                                   pack_a, pack_b, GS_CULL_TAIL);
            else if (packed)
                hipLaunchKernelGGL(frame_packed_project_cull_count_kernel, dim3(nsl + 1), dim3(STRIP_THREADS), lds, stream, pack_a,
                                   pack_b, GS_CULL_TAIL);
            else if (P.pp)
                hipLaunchKernelGGL(frame_project_cull_count_pp_kernel, dim3(nsl + 1), dim3(STRIP_THREADS), lds, stream, f->pos,
                                   (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_CULL_TAIL);
            else
                hipLaunchKernelGGL(frame_project_cull_count_kernel, dim3(nsl + 1), dim3(STRIP_THREADS), lds, stream, f->pos,
                                   (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_CULL_TAIL);
#undef GS_CULL_TAIL
            GS_CHECK_LAUNCH();
            return 0;
        }
        const size_t lds = sizeof(unsigned long long) * SG.NS;
        const uint32_t extra = (slice_begin == 0 && !second_pass) ? 1u : 0u;  // the tile-order workgroup rides with the first range
        const unsigned long long *gate = second_pass ? ws.counters + GS_CNT_RANPAST : nullptr;
#define GS_COUNT_TAIL                                                                                                  \
    f->N, P, ws.rec_geom, touched, ws.rects, D, plan.per_slice, SG, nsl, (uint32_t)slice_begin, table, ws.slice_pairs, \
        ws.slice_vis, ws.tile_cost, (uint32_t)G.n_tiles, ws.tile_order, gate
#define GS_LAUNCH_PROJECT_COUNT(DIST)                                                                                  \
    do {                                                                                                               \
        if (cam_dev && P.pp)                                                                                           \
            hipLaunchKernelGGL(frame_project_count_pp_dp_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds, stream, \
                               cam_dev, f->pos, (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_COUNT_TAIL);     \
        else if (cam_dev)                                                                                              \
            hipLaunchKernelGGL(frame_project_count_dp_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds, stream, \
                               cam_dev, f->pos, (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_COUNT_TAIL);     \
        else if (packed && P.pp)                                                                                       \
            hipLaunchKernelGGL(frame_packed_project_count_pp_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds, \
                               stream, pack_b, GS_COUNT_TAIL);                                                         \
        else if (packed)                                                                                               \
            hipLaunchKernelGGL(frame_packed_project_count_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds,   \
                               stream, pack_b, GS_COUNT_TAIL);                                                         \
        else if (P.pp)                                                                                                 \
            hipLaunchKernelGGL(frame_project_count_pp_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds, stream, \
                               f->pos, (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_COUNT_TAIL);              \
        else                                                                                                           \
            hipLaunchKernelGGL(frame_project_count_kernel<DIST>, dim3(nsl + extra), dim3(STRIP_THREADS), lds, stream,  \
                               f->pos, (const float4 *)f->quat, f->scale, f->opa, f->rgb, GS_COUNT_TAIL);              \
    } while (0)
        if (f->tile_culling_method == 0)
            GS_LAUNCH_PROJECT_COUNT(true);
        else
            GS_LAUNCH_PROJECT_COUNT(false);
#undef GS_LAUNCH_PROJECT_COUNT
#undef GS_COUNT_TAIL
        GS_CHECK_LAUNCH();
        return 0;
    }
    GS_CHECK_ARG(!second_pass, "the second pass of an occlusion-culled frame belongs to the strip variant's project + count stage");
    GS_CHECK_ARG(slice_begin == 0 && slice_end < 0, "this frame's project stage cannot be issued in ranges");
    if (gs_frame_fused_table_count(f)) {
        gs_frame_geom G = gs_frame_geometry(f);
        const GsDistCull D = gs_frame_dist_cull(f);
        static std::mutex attr_mu2;
        static std::atomic<uint64_t> attr_done2{0};
        int dev = 0;
        GS_HIP(hipGetDevice(&dev));
        if (dev < 64 && !((attr_done2.load(std::memory_order_acquire) >> dev) & 1)) {
            std::lock_guard<std::mutex> lock(attr_mu2);
            for (const void *fn : {(const void *)frame_project_bin_count_kernel<false>, (const void *)frame_project_bin_count_kernel<true>,
                                   (const void *)frame_project_bin_count_pp_kernel<false>,
                                   (const void *)frame_project_bin_count_pp_kernel<true>,
                                   (const void *)frame_project_bin_count_dp_kernel<false>, (const void *)frame_project_bin_count_dp_kernel<true>,
                                   (const void *)frame_project_bin_count_pp_dp_kernel<false>,
                                   (const void *)frame_project_bin_count_pp_dp_kernel<true>})
                GS_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, GS_BIN_MAX_TILES * 4));
            attr_done2.fetch_or(1ull << dev, std::memory_order_release);
        }
        const uint32_t per_block = bin_per_block(f->N), B = (uint32_t)gs_div_up(f->N, per_block);
        const uint32_t T = (uint32_t)G.n_tiles;
        const Cam *cam_dev = (const Cam *)gs_frame_pose_dev(f);  // GS_FRAME_DEVICE_POSE: the *_dp_kernel twins
#define GS_BIN_TAIL                                                                                                    \
    f->pos, (const float4 *)f->quat, f->scale, f->opa, f->rgb, f->N, P, ws.rec_geom, ws.rects, D, per_block, T,        \
        ws.bin_table, ws.slice_pairs, ws.slice_vis
#define GS_LAUNCH_PROJECT_BIN_K(KERNEL)                                                                                \
    hipLaunchKernelGGL(KERNEL, dim3(B), dim3(BIN_THREADS), sizeof(uint32_t) * T, stream, GS_BIN_TAIL)
#define GS_LAUNCH_PROJECT_BIN_DP(KERNEL)                                                                               \
    hipLaunchKernelGGL(KERNEL, dim3(B), dim3(BIN_THREADS), sizeof(uint32_t) * T, stream, cam_dev, GS_BIN_TAIL)
#define GS_LAUNCH_PROJECT_BIN(DIST)                                                                                    \
    do {                                                                                                               \
        if (cam_dev && P.pp)                                                                                           \
            GS_LAUNCH_PROJECT_BIN_DP(frame_project_bin_count_pp_dp_kernel<DIST>);                                      \
        else if (cam_dev)                                                                                              \
            GS_LAUNCH_PROJECT_BIN_DP(frame_project_bin_count_dp_kernel<DIST>);                                         \
        else if (P.pp)                                                                                                 \
            GS_LAUNCH_PROJECT_BIN_K(frame_project_bin_count_pp_kernel<DIST>);                                          \
        else                                                                                                           \
            GS_LAUNCH_PROJECT_BIN_K(frame_project_bin_count_kernel<DIST>);                                             \
    } while (0)
        if (f->tile_culling_method == 0)
            GS_LAUNCH_PROJECT_BIN(true);
        else
            GS_LAUNCH_PROJECT_BIN(false);
#undef GS_LAUNCH_PROJECT_BIN
#undef GS_LAUNCH_PROJECT_BIN_K
#undef GS_LAUNCH_PROJECT_BIN_DP
#undef GS_BIN_TAIL
        GS_CHECK_LAUNCH();
        return 0;
    }
    int nblk = (int)gs_div_up(f->N, 256);
    if (P.pp)
        hipLaunchKernelGGL(frame_project_pp_kernel, dim3(nblk), dim3(256), 0, stream, f->pos, (const float4 *)f->quat,
                           f->scale, f->opa, f->rgb, f->N, P, ws.rec_geom,
                           touched, ws.rects, ws.block_sums, ws.block_vis);
    else
        hipLaunchKernelGGL(frame_project_kernel, dim3(nblk), dim3(256), 0, stream, f->pos, (const float4 *)f->quat,
                           f->scale, f->opa, f->rgb, f->N, P, ws.rec_geom,
                           touched, ws.rects, ws.block_sums, ws.block_vis);
    GS_CHECK_LAUNCH();
    return 0;
}
