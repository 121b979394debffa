// project_bwd.hip -- backward of the projection (cull_project.hip, project_common.h), and the fused Adam step behind it.
//
// Replaces global_culling_backward_kernel (gaussian.cu:1371-1576) of the reference, and provides the last stage of the frame
// path (gs_frame_backward and its variants): the gradient rows the raster backward left are summed per Gaussian in a fixed
// order and pushed through the projection + activation backward -- with the pose gradient's partial sums
// (GS_FRAME_POSE_GRAD), the depth map's position term (GS_FRAME_AUX) or the optimizer step (gs_frame_backward_adam) in
// the same pass or right behind it.  The kernel bodies are frame_project_backward_body.inc, aux_depth_backward_body.inc
// and aux_depth_term.inc, expanded in place.
//
// This file is compiled with -ffp-contract=off: its outputs are pinned bit for bit by the golden tests, the fused step
// must round like adam.hip (gs_adam_one), and the AUX position term is fl(gp) + gpa in that order, which is what
// gs_frame_backward followed by the aux depth kernel leaves.  Contraction is switched on by pragma exactly where a
// tolerance allows it (project_backward, pose_terms).
#include <type_traits>

#include "gs_common.h"
#include "gs_frame_layout.h"
#include "project_common.h"

namespace {

// Backward of `project` w.r.t. (p, q_hat, s_hat) given dL/dpos_i and dL/dcov
// (gaussian.cu:1393-1575; the dependence of J on p is dropped exactly as there).
// Unlike the forward (depth bits and tile rectangles must equal the oracle's bit for bit: cull_project.hip evaluates
// every expression uncontracted), gradients are compared within a tolerance: everything between the two pragmas contracts
// to FMAs, and the backward uses v_rcp_f32 / v_rsq_f32 (1 ulp) for its reciprocals -- seven correctly rounded divisions, a
// square root and ~150 separate multiplies and adds were a third of the projection backward's instructions (round 4: the
// kernel turned out to be VALU-bound, not HBM-bound, once it stopped fetching rows nobody wrote).
#pragma clang fp contract(fast)
__device__ __forceinline__ void project_backward(const float p[3], const float q[4], const float s[3],
                                                 const Cam &cam, const float gi[3], const float g2[4],
                                                 float gp[3], float gq[4], float gs[3]) {
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = cam.rot[r * 3 + 0] * p[0] + cam.rot[r * 3 + 1] * p[1] + cam.rot[r * 3 + 2] * p[2] + cam.tran[r];
    const float ir_ = gs_rsq(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]), iz = gs_rcp(pc[2]);
    float gc[3];
    gc[0] = gi[0] * iz + gi[2] * pc[0] * ir_;
    gc[1] = gi[1] * iz + gi[2] * pc[1] * ir_;
    gc[2] = -(gi[0] * pc[0] + gi[1] * pc[1]) * (iz * iz) + gi[2] * pc[2] * ir_;
#pragma unroll
    for (int ir = 0; ir < 3; ++ir) {
        float a = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) a += cam.rot[k * 3 + ir] * gc[k];
        gp[ir] = a;
    }
    // rows 0, 1 of J W (J = [[1/z, 0, -x/z^2], [0, 1/z, -y/z^2]])
    float JW[6];
    const float jx = -pc[0] * (iz * iz), jy = -pc[1] * (iz * iz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        JW[c] = iz * cam.rot[c] + jx * cam.rot[6 + c];
        JW[3 + c] = iz * cam.rot[3 + c] + jy * cam.rot[6 + c];
    }
    float g3[9];
#pragma unroll
    for (int ir = 0; ir < 3; ++ir)
#pragma unroll
        for (int ic = 0; ic < 3; ++ic) {
            float a = 0;
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int ij = 0; ij < 2; ++ij) a += g2[ii * 2 + ij] * JW[ii * 3 + ir] * JW[ij * 3 + ic];
            g3[ir * 3 + ic] = a;
        }
    float R[9], RS[9], gRS[9];
    quat_to_R(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int i = 0; i < 9; ++i) RS[i] = R[i] * s[i % 3];
#pragma unroll
    for (int ir = 0; ir < 3; ++ir)
#pragma unroll
        for (int ic = 0; ic < 3; ++ic) {
            float a = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) a += (g3[k * 3 + ir] + g3[ir * 3 + k]) * RS[k * 3 + ic];
            gRS[ir * 3 + ic] = a;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        gs[i] = gRS[0 * 3 + i] * R[0 * 3 + i] + gRS[1 * 3 + i] * R[1 * 3 + i] + gRS[2 * 3 + i] * R[2 * 3 + i];
    const float sx = s[0], sy = s[1], sz = s[2];
    const float qr = q[0], qi = q[1], qj = q[2], qk = q[3];
    const float c_qr[9] = {0, -2 * sy * qk, 2 * sz * qj, 2 * sx * qk, 0, -2 * sz * qi, -2 * sx * qj, 2 * sy * qi, 0};
    const float c_qi[9] = {0, 2 * sy * qj, 2 * sz * qk, 2 * sx * qj, -4 * sy * qi, -2 * sz * qr,
                           2 * sx * qk, 2 * sy * qr, -4 * sz * qi};
    const float c_qj[9] = {-4 * sx * qj, 2 * sy * qi, 2 * sz * qr, 2 * sx * qi, 0, 2 * sz * qk,
                           -2 * sx * qr, 2 * sy * qk, -4 * sz * qj};
    const float c_qk[9] = {-4 * sx * qk, -2 * sy * qr, 2 * sz * qi, 2 * sx * qr, -4 * sy * qk, 2 * sz * qj,
                           2 * sx * qi, 2 * sy * qj, 0};
    float a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    {
        // NOT contracted: for an isotropic Gaussian the rotation has no effect and these sums are +p - p with both
        // products rounded alike, i.e. exactly zero (COLMAP-initialised scenes are all isotropic); an fma would leave the
        // rounding error of one product as a "gradient" (tests/test_gpu_splatter.py caught 5e-8 against an exact 0)
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            a0 += c_qr[i] * gRS[i];
            a1 += c_qi[i] * gRS[i];
            a2 += c_qj[i] * gRS[i];
            a3 += c_qk[i] * gRS[i];
        }
    }
    gq[0] = a0;
    gq[1] = a1;
    gq[2] = a2;
    gq[3] = a3;
}

// GS_FRAME_POSE_GRAD: one visible Gaussian's share of dL/d(rot) [3x3, row-major] and dL/d(tran) [3] -> t[0..8], t[9..11], from
// the same inputs as project_backward (which already forms gc = dL/dp_c and JW; the recomputation is the same expressions
// and folds into it).  With p_c = rot p + tran and cov2d = J rot C rot^T J^T, C = (R S)(R S)^T, J held fixed as above:
//   dL/dtran = gc,   dL/drot = gc p^T + J^T (G + G^T) J rot C,   G = dL/dcov2d (g2: G00, G01, G10, G11).
// J^T (G + G^T) J rot C = J^T K (RS)(RS)^T with K = (G + G^T) (J rot) [2x3]: ~80 FMAs.
// U0_EXPLICIT (the AUX variants of the fused step and of the pose-only kernel, no other): everything here contracts by pragma,
// and which product of a b + c d the compiler fuses follows the operand order its optimizer leaves, which depends on the code
// around the call.  In every other kernel that expands this function U[a][0] comes out as fma(K2, RS6, fma(K1, RS3, fl(K0 RS0))); with the depth map's
// row walk in the same kernel the first two products change places -- the one sum of this function that moves, found by
// comparing the kernels' machine code -- and the pose row loses its last bit against frame_project_backward_pose_kernel.
// The flag states that sum the way the other kernels have it.  tests/test_gpu_pose_adam.py compares the rows bit for bit.
// frame_pose_backward_kernel<true> met the same thing without project_backward around the call (one row entry of 24 lost its
// last bit at N = 37; with the flag every row of tests/test_gpu_pose_only.py is equal); its plain variant needs no help.
template <bool U0_EXPLICIT = false>
__device__ __forceinline__ void pose_terms(const float p[3], const float q[4], const float s[3], const Cam &cam,
                                           const float gi[3], const float g2[4], float t[12]) {
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = cam.rot[r * 3 + 0] * p[0] + cam.rot[r * 3 + 1] * p[1] + cam.rot[r * 3 + 2] * p[2] + cam.tran[r];
    const float ir_ = gs_rsq(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]), iz = gs_rcp(pc[2]);
    float gc[3];
    gc[0] = gi[0] * iz + gi[2] * pc[0] * ir_;
    gc[1] = gi[1] * iz + gi[2] * pc[1] * ir_;
    gc[2] = -(gi[0] * pc[0] + gi[1] * pc[1]) * (iz * iz) + gi[2] * pc[2] * ir_;
    float JW[6];
    const float jx = -pc[0] * (iz * iz), jy = -pc[1] * (iz * iz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        JW[c] = iz * cam.rot[c] + jx * cam.rot[6 + c];
        JW[3 + c] = iz * cam.rot[3 + c] + jy * cam.rot[6 + c];
    }
    const float h00 = g2[0] + g2[0], h01 = g2[1] + g2[2], h11 = g2[3] + g2[3];
    float K[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        K[c] = h00 * JW[c] + h01 * JW[3 + c];
        K[3 + c] = h01 * JW[c] + h11 * JW[3 + c];
    }
    float R[9], RS[9];
    quat_to_R(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int i = 0; i < 9; ++i) RS[i] = R[i] * s[i % 3];
    float U[6], KC[6];  // U = K RS, KC = U RS^T = K C
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (U0_EXPLICIT && k == 0) {
                const float first = K[a * 3 + 0] * RS[0];
                U[a * 3] = __builtin_fmaf(K[a * 3 + 2], RS[6], __builtin_fmaf(K[a * 3 + 1], RS[3], first));
            } else {
                U[a * 3 + k] = K[a * 3 + 0] * RS[0 * 3 + k] + K[a * 3 + 1] * RS[1 * 3 + k] + K[a * 3 + 2] * RS[2 * 3 + k];
            }
        }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) KC[a * 3 + c] = U[a * 3 + 0] * RS[c * 3 + 0] + U[a * 3 + 1] * RS[c * 3 + 1] + U[a * 3 + 2] * RS[c * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // J^T KC: J = [[iz, 0, jx], [0, iz, jy]]
        t[0 * 3 + c] = gc[0] * p[c] + iz * KC[c];
        t[1 * 3 + c] = gc[1] * p[c] + iz * KC[3 + c];
        t[2 * 3 + c] = gc[2] * p[c] + (jx * KC[c] + jy * KC[3 + c]);
    }
    t[9] = gc[0];
    t[10] = gc[1];
    t[11] = gc[2];
}
#pragma clang fp contract(off)

// GS_FRAME_POSE_GRAD: the workgroup's sum of every thread's 12 pose terms -> row[0..11] (one row per workgroup, summed by
// pose_grad_finalize_kernel).  A fixed order, no atomics -- bitwise repeatable like every other gradient here: a butterfly
// over the wave (both partners add the same two values: every lane holds the same bits), then the waves in index order.
// Every thread of the workgroup must call it.  SLOT: a kernel that sums two rows (the fused step's AUX + POSE variant) gives
// each its own LDS array, so the second sum's writes cannot overtake the first one's reads.
template <int BLOCK, int SLOT = 0>
__device__ __forceinline__ void pose_block_sum(float t[12], float *__restrict__ row) {
    __shared__ float s_pose[BLOCK / 64][12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[e] += __shfl_xor(t[e], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) s_pose[threadIdx.x >> 6][e] = t[e];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        float a = s_pose[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) a += s_pose[w][threadIdx.x];
        row[threadIdx.x] = a;
    }
}

// ---------------------------------------------------------------- reference-API kernel
__global__ void __launch_bounds__(256) global_culling_backward_kernel(
    const float *__restrict__ pos, const float4 *__restrict__ quat, const float *__restrict__ scale,
    const float *__restrict__ rot, const float *__restrict__ tran, int64_t n,
    const float *__restrict__ gradout_pos, const float4 *__restrict__ gradout_cov,
    const int64_t *__restrict__ mask, float *__restrict__ gin_pos, float4 *__restrict__ gin_quat,
    float *__restrict__ gin_scale) {
    Cam cam;
#pragma unroll
    for (int i = 0; i < 9; ++i) cam.rot[i] = rot[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) cam.tran[i] = tran[i];
    for (int64_t pid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < n;
         pid += (int64_t)gridDim.x * blockDim.x) {
        if (mask[pid] == 0) continue;
        float p[3], s[3], gi[3], gp[3], gq[4], gs[3];
        load3(pos, pid, p);
        load3(scale, pid, s);
        load3(gradout_pos, pid, gi);
        float4 q4 = quat[pid], c4 = gradout_cov[pid];
        float q[4] = {q4.x, q4.y, q4.z, q4.w}, g2[4] = {c4.x, c4.y, c4.z, c4.w};
        project_backward(p, q, s, cam, gi, g2, gp, gq, gs);
        gin_pos[pid * 3 + 0] = gp[0];
        gin_pos[pid * 3 + 1] = gp[1];
        gin_pos[pid * 3 + 2] = gp[2];
        gin_quat[pid] = make_float4(gq[0], gq[1], gq[2], gq[3]);
        gin_scale[pid * 3 + 0] = gs[0];
        gin_scale[pid * 3 + 1] = gs[1];
        gin_scale[pid * 3 + 2] = gs[2];
    }
}

// ---------------------------------------------------------------- fused frame stage B2
// rows[pair][12|36|56] = (dx, dy, da, db, dc, dd, dopa, colour grads..) written by the raster backward
// in emission order: Gaussian g owns rows [pair_offsets[g], +tiles_touched[g]).  They are summed
// here in a fixed order (the reference's index_put_(accumulate=True), but deterministic) and pushed
// through the projection + activation backward.  Culled Gaussians get zeros.  Only rows whose flag is set were written
// by the raster backward (pairs behind a tile's early-termination point are not): the others are skipped, never read
// as numbers -- they are uninitialised memory.
// PART: 0 = everything; 1 = only the projection / activation backward (grad_pos, grad_quat, grad_scale -- the
// "geometry" bucket of the view-parallel gradient exchange); 2 = only grad_opa and grad_rgb (the "colour" bucket).
// Parts 1 and 2 read the same rows and add them in the same order as part 0: their outputs are bit-identical to it.
// They exist so that the all-reduce of the first bucket can run underneath the second kernel (gs_dp.py).
// SH rows of Gaussians that cover hundreds of tiles.  The projection backward's wave walks the rows of its 64 Gaussians one
// row per load instruction; a Gaussian with thousands of rows (a blown-up scale, a background blob: every densifying run
// has a few) kept ONE wave walking for a millisecond while the rest of the device had finished -- 1.04 of the 2.9 ms of a
// training iteration in the SH soak of round 4 (376 k Gaussians, profiles/r04_zn_*).  This kernel runs once per backward,
// right behind the raster backward: a workgroup scans its slice of the rectangles, and for every Gaussian with more than
// GS_PB_SH_BIG rows its sixteen waves add a sixteenth of the Gaussian's existing rows each (ascending, lane c = float c),
// the partial sums are added in a fixed order and the TOTAL replaces the first row of the Gaussian's region.  The
// projection backward then treats such a Gaussian as having that one row (whether or not its own pair was processed), in
// every part and slice.  Deterministic: fixed partition, fixed order.  Which rows exist: the tiles' stop keys (round 5; a
// flag byte per row until then), exactly the test of the rgb reader below.
#ifndef GS_PB_SH_BIG
#define GS_PB_SH_BIG 64
#endif
template <int CDIM>
__global__ void __launch_bounds__(1024) sh_big_rows_kernel(const uint4 *__restrict__ rects,
                                                          const uint32_t *__restrict__ pair_offsets,
                                                          float *__restrict__ rows,
                                                          const unsigned long long *__restrict__ stop_keys,
                                                          const float4 *__restrict__ rec_geom, uint32_t ntx, uint32_t n_tiles,
                                                          int cull_method, GsDistCull D,
                                                          int64_t n, uint64_t max_pairs, int64_t per_block) {
    constexpr int RWF = gs_row_floats(CDIM), WAVES = 16;
    static_assert(RWF <= 64, "a row is read by one wave instruction");
    __shared__ uint8_t s_big[1024];
    __shared__ float s_part[WAVES][RWF];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t *stop_depth = reinterpret_cast<const uint32_t *>(stop_keys), *stop_id = stop_depth + n_tiles;
    const int64_t g_begin = (int64_t)blockIdx.x * per_block;
    const int64_t g_end = g_begin + per_block < n ? g_begin + per_block : n;
    for (int64_t b0 = g_begin; b0 < g_end; b0 += 1024) {  // (uniform trip count)
        const int64_t i = b0 + threadIdx.x;
        const uint4 rc = i < g_end ? rects[i] : make_uint4(0, 0, 0, 0);
        const bool big = rc.z != 0 && rc.w > (uint32_t)GS_PB_SH_BIG;
        if (!__syncthreads_or(big)) continue;  // nearly every batch
        s_big[threadIdx.x] = big ? 1 : 0;
        __syncthreads();
        for (int j = 0; j < 1024; ++j) {
            if (!s_big[j]) continue;  // uniform
            const int64_t g = b0 + j;
            const uint64_t off = pair_offsets[g];
            const uint4 grc = rects[g];  // (uniform)
            const uint32_t gy0 = grc.x & 0xffff, gx0 = grc.y & 0xffff, gw = (grc.y >> 16) - (grc.y & 0xffff);
            float gcx = 0.f, gcy = 0.f;
            if (cull_method == 0) {  // "dist": not every tile of the bounding square is listed
                const float4 gg = rec_geom[g * GS_REC_STRIDE];
                gcx = gg.x;
                gcy = gg.y;
            }
            uint64_t cnt = grc.w;
            if (off >= max_pairs) cnt = 0;
            else if (off + cnt > max_pairs) cnt = max_pairs - off;
            const uint32_t chunk = (uint32_t)((cnt + WAVES - 1) / WAVES);
            const uint32_t k1 = (uint32_t)((uint64_t)(wv + 1) * chunk < cnt ? (uint64_t)(wv + 1) * chunk : cnt);
            float acc = 0.f;
            for (uint32_t k = (uint32_t)wv * chunk; k < k1; k += 64) {
                const uint32_t kk = k + (uint32_t)lane;
                bool ex = false;
                if (kk < k1) {  // row kk = tile (gx0 + kk % gw, gy0 + kk / gw): processed iff key(g) <= the tile's stop key
                    const uint32_t iy = gy0 + kk / gw, ix = gx0 + kk % gw, t = iy * ntx + ix;
                    const uint32_t sd = stop_depth[t];
                    ex = grc.z < sd || (grc.z == sd && (uint32_t)g <= stop_id[t]);
                    if (cull_method == 0 && !gs_dist_listed(gcx, gcy, ix, iy, D)) ex = false;
                }
                unsigned long long m = __ballot(ex);
                while (m) {  // the window's existing rows in ascending order, eight loads in flight
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        v[u] = 0.f;
                        if (m) {
                            const uint32_t r = (uint32_t)__ffsll((long long)m) - 1;
                            m &= m - 1;
                            if (lane < RWF) v[u] = rows[(off + k + r) * RWF + lane];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) acc += v[u];
                }
            }
            if (lane < RWF) s_part[wv][lane] = acc;
            __syncthreads();  // every wave has read its rows (the first row among them) and left its partial sums
            if (threadIdx.x < (unsigned)RWF && cnt) {
                const int c = threadIdx.x;
                float t[WAVES];
#pragma unroll
                for (int w = 0; w < WAVES; ++w) t[w] = s_part[w][c];
#pragma unroll
                for (int st = 1; st < WAVES; st <<= 1)  // fixed pairwise tree
#pragma unroll
                    for (int w = 0; w < WAVES; w += 2 * st) t[w] += t[w + st];
                rows[off * RWF + c] = t[0];
            }
            __syncthreads();
        }
    }
}

// GS_FRAME_AUX training frames: dL/dd_i of the depth map (d_i = |p_c|, res_pos[:, 2] of global_culling) is the sum of the
// depth floats (gs_row_aux_depth) of the Gaussian's existing rows -- the same rows, in the same ascending order, the
// projection backward reads: the tiles' stop keys decide, and an SH Gaussian beyond GS_PB_SH_BIG rows has its total in its
// first row (sh_big_rows_kernel adds the depth float up with the rest) --, and it enters grad_pos as gradout_pos[:, 2] of
// global_culling_backward (gaussian.cu:1400-1406): R^T (g_d p_c / |p_c|), added to what frame_project_backward_kernel wrote.
// A kernel of its own, behind the geometry part, so that the projection backward of frames without the flag stays as it is.
// Its body (aux_depth_backward_body.inc) is shared with the GS_FRAME_POSE_GRAD variant below: POSE (rgb colours) also
// enters the depth term gc = g_d p_c / |p_c| into the pose gradient (gc p^T, gc: pose_terms), summed per workgroup into
// pose_part[blockIdx.x] -- every thread takes part, with zeros where it has no visible Gaussian.
template <int CDIM>
__global__ void __launch_bounds__(256) frame_aux_depth_backward_kernel(const float *__restrict__ pos, int64_t n, int64_t g_first,
                                                                       ProjectParams P, const float4 *__restrict__ rec_geom,
                                                                       const float *__restrict__ rows,
                                                                       const unsigned long long *__restrict__ stop_keys, GsDistCull D,
                                                                       const uint32_t *__restrict__ pair_offsets,
                                                                       const uint4 *__restrict__ rects, uint64_t max_pairs,
                                                                       float *__restrict__ grad_pos) {
    constexpr bool POSE = false;
    [[maybe_unused]] float pt[1];
#include "aux_depth_backward_body.inc"
}

// GS_FRAME_AUX + GS_FRAME_POSE_GRAD (rgb colours): the same, plus one row of pose partial sums per workgroup
__global__ void __launch_bounds__(256) frame_aux_depth_pose_backward_kernel(const float *__restrict__ pos, int64_t n,
                                                                            ProjectParams P, const float4 *__restrict__ rec_geom,
                                                                            const float *__restrict__ rows,
                                                                            const unsigned long long *__restrict__ stop_keys,
                                                                            GsDistCull D, const uint32_t *__restrict__ pair_offsets,
                                                                            const uint4 *__restrict__ rects, uint64_t max_pairs,
                                                                            float *__restrict__ grad_pos,
                                                                            float *__restrict__ pose_part) {
    constexpr int CDIM = 3;
    constexpr bool POSE = true;
    const int64_t g_first = 0;
    float pt[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) pt[e] = 0.f;
    [&]() {
#include "aux_depth_backward_body.inc"
    }();
    pose_block_sum<256>(pt, pose_part + (size_t)blockIdx.x * 12);  // (every thread: the early returns left the lambda only)
}

// GS_FRAME_POSE_GRAD: grad_rot [3,3] / grad_tran [3] = the sum of the partial rows (the projection backward's, then the aux
// depth kernel's), in double and in a fixed order -- thread t takes rows t, t + 1024, ... in ascending order, then a
// butterfly over the wave, then the waves in index order.  Overwritten, never accumulated; an overflowed frame (rendered
// empty) gets zeros.  One workgroup.
__global__ void __launch_bounds__(1024) pose_grad_finalize_kernel(const float4 *__restrict__ part, int64_t nrows,
                                                                  const unsigned long long *__restrict__ overflow,
                                                                  float *__restrict__ grad_rot, float *__restrict__ grad_tran) {
    __shared__ double s_w[16][12];
    double acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.0;
    constexpr int U = 4;  // rows in flight per thread
    int64_t r = threadIdx.x;
    for (; r + (U - 1) * 1024 < nrows; r += U * 1024) {
        float4 v[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int m = 0; m < 3; ++m) v[u][m] = part[(r + u * 1024) * 3 + m];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                acc[4 * m + 0] += (double)v[u][m].x;
                acc[4 * m + 1] += (double)v[u][m].y;
                acc[4 * m + 2] += (double)v[u][m].z;
                acc[4 * m + 3] += (double)v[u][m].w;
            }
    }
    for (; r < nrows; r += 1024) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const float4 v = part[r * 3 + m];
            acc[4 * m + 0] += (double)v.x;
            acc[4 * m + 1] += (double)v.y;
            acc[4 * m + 2] += (double)v.z;
            acc[4 * m + 3] += (double)v.w;
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) s_w[threadIdx.x >> 6][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int nw = (int)(blockDim.x >> 6);
        double a = s_w[0][threadIdx.x];
        for (int w = 1; w < nw; ++w) a += s_w[w][threadIdx.x];
        const float v = *overflow ? 0.f : (float)a;
        if (threadIdx.x < 9)
            grad_rot[threadIdx.x] = v;
        else
            grad_tran[threadIdx.x - 9] = v;
    }
}

#ifndef GS_PB_SH_PASSES
#define GS_PB_SH_PASSES 2  // A/B switch: the SH row walk in this many passes over 64 / PASSES owners each (LDS per wave)
#endif
#ifndef GS_PB_SH_U
#define GS_PB_SH_U 8  // A/B switch: row loads the SH walk keeps in flight
#endif
// The optimizer step fused into the kernel's epilogue (gs_frame_backward_adam, include/gs_abi.h; rgb colours, PART 0): instead of
// storing the Gaussian's 14 gradients the thread applies gs_adam_one to its 14 parameters -- the five raw parameter arrays
// are then written through `p_*` (the same memory the kernel read them from: every thread reads its own Gaussian's parameters
// before it overwrites them, nobody else's), the moments through m_* / v_*.  ADAM: 0 = off, 1 = plain accesses, 2 = moments
// with non-temporal loads / stores (beyond the Infinity Cache they only evict each other on their way through: adam.hip).
struct AdamFusedDev {
    float *p_pos, *p_quat, *p_scale, *p_opa, *p_rgb;
    float *m_pos, *m_quat, *m_scale, *m_opa, *m_rgb;
    float *v_pos, *v_quat, *v_scale, *v_opa, *v_rgb;
    float step_pos, step_quat, step_scale, step_opa, step_rgb;  // lr_k / (1 - b1^t)
    float one_m_b1, b2, one_m_b2, inv_bc2_sqrt, eps;
    float *stat;  // [N,3] or NULL
    int stat_mode;
    const unsigned long long *skip_if_nonzero;
};
// The rgb / SH projection backward.  Its body (frame_project_backward_body.inc) is shared with the GS_FRAME_POSE_GRAD variant
// below: POSE (rgb colours, PART 0 / 1, no fused step) does the same per-Gaussian work and stores, and also forms every
// thread's 12 pose terms in the epilogue (pose_terms) and sums them over the workgroup into pose_part[blockIdx.x]
// (pose_block_sum).  Threads past N take part in that sum with zeros.  A Gaussian summed by the whole workgroup (GS_PB_BIG)
// has its totals in its owner's d0 / d1 like any other by the time the epilogue runs.
template <int CDIM, int PART = 0, int BLOCK = (CDIM == 3 ? 256 : 128), int ADAM = 0>
__global__ void __launch_bounds__(BLOCK) frame_project_backward_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs, int64_t g_first,
    float *__restrict__ grad_pos,
    float4 *__restrict__ grad_quat, float *__restrict__ grad_scale, float *__restrict__ grad_opa,
    float *__restrict__ grad_rgb, AdamFusedDev A = AdamFusedDev{}) {
    constexpr bool POSE = false, AUX = false, POSE_ONLY = false;
    [[maybe_unused]] float *const pose_part = nullptr, *const pose_part_aux = nullptr;
#include "frame_project_backward_body.inc"
}

// GS_FRAME_AUX frames with the fused step (gs_frame_backward_adam_aux): the ADAM = 1 / 2 instantiations above with the depth
// map's position term added to gp in front of the epilogue (AUX; aux_depth_term.inc: the row walk of
// frame_aux_depth_backward_kernel).  A kernel of its own name, so that the kernels of frames without the flag keep theirs.
template <int CDIM, int BLOCK, int ADAM>
__global__ void __launch_bounds__(BLOCK) frame_project_backward_adam_aux_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs, AdamFusedDev A) {
    static_assert(ADAM != 0, "the fused step's variant");
    constexpr int PART = 0;
    constexpr bool POSE = false, AUX = true, POSE_ONLY = false;
    const int64_t g_first = 0;
    [[maybe_unused]] float *const pose_part = nullptr, *const pose_part_aux = nullptr;
    // (no gradient is stored: the names the body's unfused tail mentions)
    [[maybe_unused]] float *const grad_pos = nullptr, *const grad_scale = nullptr, *const grad_opa = nullptr, *const grad_rgb = nullptr;
    [[maybe_unused]] float4 *const grad_quat = nullptr;
#include "frame_project_backward_body.inc"
}

// GS_FRAME_POSE_GRAD frames (rgb colours): PART 0 (everything) or 1 (geometry), all Gaussians from 0, 256 threads; one row
// of 12 pose partial sums per workgroup into pose_part
template <int PART>
__global__ void __launch_bounds__(256) frame_project_backward_pose_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs,
    float *__restrict__ grad_pos,
    float4 *__restrict__ grad_quat, float *__restrict__ grad_scale, float *__restrict__ grad_opa,
    float *__restrict__ grad_rgb, float *__restrict__ pose_part) {
    constexpr int CDIM = 3, BLOCK = 256, ADAM = 0;
    constexpr bool POSE = true, AUX = false, POSE_ONLY = false;
    const int64_t g_first = 0;
    [[maybe_unused]] const AdamFusedDev A{};
    [[maybe_unused]] float *const pose_part_aux = nullptr;
#include "frame_project_backward_body.inc"
}

// GS_FRAME_POSE_GRAD training frames with the fused step (gs_frame_backward_adam_pose), plain (AUX false) or GS_FRAME_AUX: the
// ADAM = 1 / 2 step of frame_project_backward_kernel<3, 0, 256, .> / frame_project_backward_adam_aux_kernel<3, 256, .> with the
// pose terms of frame_project_backward_pose_kernel<0> -- and, AUX, of frame_aux_depth_pose_backward_kernel -- formed from the
// position, quaternion and scale the thread loaded BEFORE the step, and summed over the workgroup in front of the epilogue.
// One row of 12 partial sums per workgroup into pose_part, AUX: a second one into pose_part_aux -- the layout the two
// unfused kernels leave, so pose_grad_finalize_kernel runs as it is.  Threads past N add zeros to both sums, take part in
// the epilogue's hand-overs and leave where it lets them.  A kernel of its own name: the others keep their code.
template <bool AUX, int ADAM>
__global__ void __launch_bounds__(256) frame_project_backward_adam_pose_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs, AdamFusedDev A,
    float *__restrict__ pose_part, float *__restrict__ pose_part_aux) {
    static_assert(ADAM != 0, "the fused step's variant");
    constexpr int CDIM = 3, PART = 0, BLOCK = 256;
    constexpr bool POSE = true, POSE_ONLY = false;
    const int64_t g_first = 0;
    // (no gradient is stored: the names the body's unfused tail mentions)
    [[maybe_unused]] float *const grad_pos = nullptr, *const grad_scale = nullptr, *const grad_opa = nullptr, *const grad_rgb = nullptr;
    [[maybe_unused]] float4 *const grad_quat = nullptr;
#include "frame_project_backward_body.inc"
}

// GS_FRAME_POSE_GRAD frames whose per-Gaussian gradients nobody reads (gs_frame_backward_pose: camera tracking against a
// frozen map), plain (AUX false) or GS_FRAME_AUX: the row sums of frame_project_backward_pose_kernel<1> and its pose terms --
// and, AUX, those of frame_aux_depth_pose_backward_kernel, with g_d taken from the same row walk -- summed over the workgroup
// into pose_part / pose_part_aux, the layout those two kernels leave, so pose_grad_finalize_kernel runs as it is.  No
// projection backward, no activation backward, no colour part; nothing is stored per Gaussian and there is no gradient
// destination.  Threads past N and culled Gaussians add zeros to both sums.  A kernel of its own name: the others keep
// their code.  (rec_color, opa_raw and rgb_raw are the launch's common arguments; not read.)
template <bool AUX>
__global__ void __launch_bounds__(256) frame_pose_backward_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs,
    float *__restrict__ pose_part, float *__restrict__ pose_part_aux) {
    constexpr int CDIM = 3, PART = 1, BLOCK = 256, ADAM = 0;
    constexpr bool POSE = true, POSE_ONLY = true;
    const int64_t g_first = 0;
    [[maybe_unused]] const AdamFusedDev A{};
    // (no gradient is stored: the names the body's unfused tail mentions)
    [[maybe_unused]] float *const grad_pos = nullptr, *const grad_scale = nullptr, *const grad_opa = nullptr, *const grad_rgb = nullptr;
    [[maybe_unused]] float4 *const grad_quat = nullptr;
#include "frame_project_backward_body.inc"
}

// GS_FRAME_DEVICE_POSE: frame_pose_backward_kernel's twin whose pose is the 12 floats `cam_dev` points to as they stand when the
// kernel runs (a uniform 48-byte load; the caller's promise: what the frame's forward read) instead of the descriptor's -- P.cam is
// replaced, the body is the same include.  A kernel of its own name: the others keep their code.
template <bool AUX>
__global__ void __launch_bounds__(256) frame_pose_backward_dp_kernel(
    const float *pos, const float4 *quat, const float *scale,
    int64_t n, ProjectParams P, const float4 *__restrict__ rec_geom,
    const float4 *__restrict__ rec_color, const float4 *__restrict__ rows,
    const unsigned long long *__restrict__ stop_keys, const float *opa_raw,
    const float *rgb_raw, GsDistCull D,
    const uint32_t *__restrict__ pair_offsets, const uint4 *__restrict__ rects, uint64_t max_pairs,
    float *__restrict__ pose_part, float *__restrict__ pose_part_aux, const Cam *__restrict__ cam_dev) {
    constexpr int CDIM = 3, PART = 1, BLOCK = 256, ADAM = 0;
    constexpr bool POSE = true, POSE_ONLY = true;
    const int64_t g_first = 0;
    [[maybe_unused]] const AdamFusedDev A{};
    // (no gradient is stored: the names the body's unfused tail mentions)
    [[maybe_unused]] float *const grad_pos = nullptr, *const grad_scale = nullptr, *const grad_opa = nullptr, *const grad_rgb = nullptr;
    [[maybe_unused]] float4 *const grad_quat = nullptr;
    P.cam = *cam_dev;
#include "frame_project_backward_body.inc"
}

}  // namespace

// ================================================================= C ABI (section A)
extern "C" int gs_global_culling_backward(const float *pos, const float *quat, const float *scale,
                                          const float *rot, const float *tran, int64_t N,
                                          const float *gradout_pos, const float *gradout_cov,
                                          const int64_t *culling_mask, float *gradinput_pos,
                                          float *gradinput_quat, float *gradinput_scale, gs_stream_t stream) {
    GS_CHECK_ARG(N >= 0, "N < 0");
    if (N == 0) return 0;
    GS_CHECK_ARG(pos && quat && scale && rot && tran && gradout_pos && gradout_cov && culling_mask &&
                     gradinput_pos && gradinput_quat && gradinput_scale,
                 "null pointer");
    GS_CHECK_ARG(((uintptr_t)quat & 15) == 0 && ((uintptr_t)gradout_cov & 15) == 0 &&
                     ((uintptr_t)gradinput_quat & 15) == 0,
                 "quat/gradout_cov/gradinput_quat must be 16-byte aligned");
    hipLaunchKernelGGL(global_culling_backward_kernel, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream,
                       pos, (const float4 *)quat, scale, rot, tran, N, gradout_pos, (const float4 *)gradout_cov,
                       culling_mask, gradinput_pos, (float4 *)gradinput_quat, gradinput_scale);
    GS_CHECK_LAUNCH();
    return 0;
}

// ================================================================= frame stages (internal)
// One launch of frame_project_backward_kernel, frame_project_backward_adam_aux_kernel, frame_project_backward_pose_kernel,
// frame_project_backward_adam_pose_kernel or frame_pose_backward_kernel over the Gaussians below `n`: the arguments they have in
// common, then `tail` (what each takes behind max_pairs).
template <class Kernel, class... Tail>
static void launch_project_backward(Kernel kernel, unsigned grid, int block, hipStream_t stream, const gs_frame *f,
                                    const gs_frame_ws &ws, int64_t n, Tail... tail) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, f->pos, (const float4 *)f->quat, f->scale, n, make_params(f),
                       ws.rec_geom, ws.rec_color, (const float4 *)ws.rows, (const unsigned long long *)ws.stop_keys, f->opa,
                       f->rgb, gs_frame_dist_cull(f), ws.pair_offsets, ws.rects, (uint64_t)f->max_pairs, tail...);
}

// SH frames, once per backward, behind the raster backward: the rows of Gaussians beyond GS_PB_SH_BIG rows are summed
// by whole workgroups (sh_big_rows_kernel)
int gs_stage_sh_big_rows(const gs_frame *f, const gs_frame_ws &ws, hipStream_t stream) {
    if (f->color_dim == 3 || f->N <= 0) return 0;
    const int blocks = 512;
    const int64_t per_block = gs_div_up(f->N, blocks);  // (the kernel walks its slice 1,024 Gaussians at a time)
    const gs_frame_geom G = gs_frame_geometry(f);
    gs_for_color_dim(f->color_dim, [&](auto cd) {
        constexpr int CD = decltype(cd)::value;
        if constexpr (CD != 3)  // (rgb frames returned above: no such kernel)
            hipLaunchKernelGGL(sh_big_rows_kernel<CD>, dim3(blocks), dim3(1024), 0, stream, ws.rects, ws.pair_offsets, ws.rows,
                               (const unsigned long long *)ws.stop_keys, ws.rec_geom, (uint32_t)G.ntx, (uint32_t)G.n_tiles,
                               f->tile_culling_method, gs_frame_dist_cull(f), f->N, (uint64_t)f->max_pairs, per_block);
    });
    GS_CHECK_LAUNCH();
    return 0;
}

// Gaussians [g_begin, g_end) only (g_begin a multiple of 256; the whole array: 0, N): the view-parallel exchange sums
// the rows slice by slice, so that a slice's gradients travel while the next slice is summed (gs_dp.py).
int gs_stage_aux_depth_backward(const gs_frame *f, const gs_frame_ws &ws, float *grad_pos, int64_t g_begin, int64_t g_end,
                                hipStream_t stream) {
    if (g_end <= g_begin) return 0;
    const unsigned grid = (unsigned)gs_div_up(g_end - g_begin, 256);
    gs_for_color_dim(f->color_dim, [&](auto cd) {
        hipLaunchKernelGGL(frame_aux_depth_backward_kernel<decltype(cd)::value>, dim3(grid), dim3(256), 0, stream, f->pos,
                           g_end, g_begin, make_params(f), ws.rec_geom, ws.rows, (const unsigned long long *)ws.stop_keys,
                           gs_frame_dist_cull(f), ws.pair_offsets, ws.rects, (uint64_t)f->max_pairs, grad_pos);
    });
    GS_CHECK_LAUNCH();
    return 0;
}

int gs_stage_aux_depth_pose_backward(const gs_frame *f, const gs_frame_ws &ws, float *grad_pos, hipStream_t stream) {
    if (f->N <= 0) return 0;
    const gs_frame_pose_ws pw = gs_frame_pose_carve(f->pose_workspace, f->N);
    hipLaunchKernelGGL(frame_aux_depth_pose_backward_kernel, dim3((unsigned)pw.rows), dim3(256), 0, stream, f->pos, f->N,
                       make_params(f), ws.rec_geom, ws.rows, (const unsigned long long *)ws.stop_keys, gs_frame_dist_cull(f),
                       ws.pair_offsets, ws.rects, (uint64_t)f->max_pairs, grad_pos, pw.aux);
    GS_CHECK_LAUNCH();
    return 0;
}

int gs_stage_project_backward_pose(const gs_frame *f, const gs_frame_ws &ws, float *grad_pos, float *grad_quat,
                                   float *grad_scale, float *grad_opa, float *grad_rgb, int part, hipStream_t stream) {
    if (f->N <= 0) return 0;
    const gs_frame_pose_ws pw = gs_frame_pose_carve(f->pose_workspace, f->N);
    auto launch = [&](auto pt) {
        launch_project_backward(frame_project_backward_pose_kernel<decltype(pt)::value>, (unsigned)pw.rows, 256, stream, f, ws,
                                f->N, grad_pos, (float4 *)grad_quat, grad_scale, grad_opa, grad_rgb, pw.proj);
    };
    if (part == 1)
        launch(gs_int<1>{});
    else
        launch(gs_int<0>{});
    GS_CHECK_LAUNCH();
    return 0;
}

// The pose gradient's partial rows alone (frame_pose_backward_kernel): one row per workgroup into pw.proj, GS_FRAME_AUX a
// second one into pw.aux -- what gs_stage_project_backward_pose(part 1) + gs_stage_aux_depth_pose_backward leave, bit for bit
int gs_stage_pose_only_backward(const gs_frame *f, const gs_frame_ws &ws, hipStream_t stream) {
    if (f->N <= 0) return 0;
    const gs_frame_pose_ws pw = gs_frame_pose_carve(f->pose_workspace, f->N);
    // GS_FRAME_DEVICE_POSE: the twin, the pose pointer as its tail argument
    const Cam *cam_dev = (const Cam *)gs_frame_pose_dev(f);
    if (cam_dev && (f->flags & GS_FRAME_AUX))
        launch_project_backward(frame_pose_backward_dp_kernel<true>, (unsigned)pw.rows, 256, stream, f, ws, f->N, pw.proj, pw.aux,
                                cam_dev);
    else if (cam_dev)
        launch_project_backward(frame_pose_backward_dp_kernel<false>, (unsigned)pw.rows, 256, stream, f, ws, f->N, pw.proj, pw.aux,
                                cam_dev);
    else if (f->flags & GS_FRAME_AUX)
        launch_project_backward(frame_pose_backward_kernel<true>, (unsigned)pw.rows, 256, stream, f, ws, f->N, pw.proj, pw.aux);
    else
        launch_project_backward(frame_pose_backward_kernel<false>, (unsigned)pw.rows, 256, stream, f, ws, f->N, pw.proj, pw.aux);
    GS_CHECK_LAUNCH();
    return 0;
}

int gs_stage_pose_finalize(const gs_frame *f, const gs_frame_ws &ws, hipStream_t stream) {
    const gs_frame_pose_ws pw = gs_frame_pose_carve(f->pose_workspace, f->N);
    const int64_t nrows = pw.rows * ((f->flags & GS_FRAME_AUX) ? 2 : 1);
    hipLaunchKernelGGL(pose_grad_finalize_kernel, dim3(1), dim3(1024), 0, stream, (const float4 *)pw.proj, nrows,
                       (const unsigned long long *)(ws.counters + GS_CNT_OVERFLOW), f->grad_rot, f->grad_tran);
    GS_CHECK_LAUNCH();
    return 0;
}

// The projection backward with the Adam step in its epilogue (gs_frame_backward_adam): rgb colours, all Gaussians, one launch
// Everything gs_frame_backward_adam can reject about its optimizer argument, checked BEFORE anything is enqueued (ADVICE
// round 5: a call rejected behind the raster backward left the caller's step counter ahead of the moments).
int gs_validate_adam_fused(const gs_frame *f, const gs_adam_fused *a) {
    GS_CHECK_ARG(f->color_dim == 3 || f->color_dim == 27 || f->color_dim == 48, "color_dim must be 3, 27 or 48");
    GS_CHECK_ARG(a->step >= 1, "step counts from 1 (torch.optim.Adam increments before the update)");
    GS_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f, "bad hyper-parameters");
    GS_CHECK_ARG(a->stat_mode >= 0 && a->stat_mode <= 2 && (!a->stat_mode || a->grad_stat), "bad statistic");
    for (int k = 0; k < 5; ++k) GS_CHECK_ARG(a->exp_avg[k] && a->exp_avg_sq[k], "null moment pointer");
    {  // the kernel walks the arrays float4 by float4
        const void *al[] = {f->pos, f->quat, f->scale, f->rgb, a->exp_avg[0], a->exp_avg[1], a->exp_avg[2], a->exp_avg[4],
                            a->exp_avg_sq[0], a->exp_avg_sq[1], a->exp_avg_sq[2], a->exp_avg_sq[4], a->grad_stat};
        for (const void *q : al) GS_CHECK_ARG(((uintptr_t)q & 15) == 0, "parameters, moments and statistic must be 16-byte aligned");
    }
    return 0;
}

int gs_stage_project_backward_adam(const gs_frame *f, const gs_frame_ws &ws, const gs_adam_fused *a, hipStream_t stream) {
    // (no gs_validate_adam_fused here: every caller has run it, before it enqueued the raster backward)
    // aux: the variant that adds the depth map's position term in front of the step (gs_frame_backward_adam_aux);
    // pose: the partial rows of the pose gradient with the step (gs_frame_backward_adam_pose), one row (aux: two) per workgroup
    const bool aux = (f->flags & GS_FRAME_AUX) != 0, pose = (f->flags & GS_FRAME_POSE_GRAD) != 0;
    GS_CHECK_ARG(!pose || f->color_dim == 3, "the fused step with a pose gradient needs rgb colours");
    if (f->N <= 0) return 0;
    const gs_frame_pose_ws pw = gs_frame_pose_carve(pose ? f->pose_workspace : nullptr, f->N);
    // bias corrections on the host in double, as torch does (adam.hip: adam_step_impl)
    const double bc1 = 1.0 - pow((double)a->beta1, (double)a->step), bc2 = 1.0 - pow((double)a->beta2, (double)a->step);
    AdamFusedDev A;
    A.p_pos = const_cast<float *>(f->pos);
    A.p_quat = const_cast<float *>(f->quat);
    A.p_scale = const_cast<float *>(f->scale);
    A.p_opa = const_cast<float *>(f->opa);
    A.p_rgb = const_cast<float *>(f->rgb);
    A.m_pos = a->exp_avg[0]; A.m_quat = a->exp_avg[1]; A.m_scale = a->exp_avg[2]; A.m_opa = a->exp_avg[3]; A.m_rgb = a->exp_avg[4];
    A.v_pos = a->exp_avg_sq[0]; A.v_quat = a->exp_avg_sq[1]; A.v_scale = a->exp_avg_sq[2]; A.v_opa = a->exp_avg_sq[3]; A.v_rgb = a->exp_avg_sq[4];
    A.step_pos = (float)((double)a->lr[0] / bc1);
    A.step_quat = (float)((double)a->lr[1] / bc1);
    A.step_scale = (float)((double)a->lr[2] / bc1);
    A.step_opa = (float)((double)a->lr[3] / bc1);
    A.step_rgb = (float)((double)a->lr[4] / bc1);
    A.one_m_b1 = 1.0f - a->beta1;
    A.b2 = a->beta2;
    A.one_m_b2 = 1.0f - a->beta2;
    A.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    A.eps = a->eps;
    A.stat = a->grad_stat;
    A.stat_mode = a->stat_mode;
    A.skip_if_nonzero = (const unsigned long long *)a->skip_if_nonzero;
    // (11 + C) parameters x 16 bytes of arrays: beyond the Infinity Cache the moments stream with non-temporal accesses (adam.hip)
    const bool nt = (unsigned long long)f->N * (unsigned long long)(11 + f->color_dim) * 16ull > (300ull << 20);
    gs_for_color_dim(f->color_dim, [&](auto cd) {
        constexpr int CD = decltype(cd)::value, BLK = CD == 3 ? 256 : 128;
        const unsigned grid = (unsigned)gs_div_up(f->N, BLK);
        auto launch = [&](auto mode) {
            constexpr int MODE = decltype(mode)::value;
            if (pose) {
                if constexpr (CD == 3) {
                    if (aux)
                        launch_project_backward(frame_project_backward_adam_pose_kernel<true, MODE>, grid, BLK, stream, f, ws,
                                                f->N, A, pw.proj, pw.aux);
                    else
                        launch_project_backward(frame_project_backward_adam_pose_kernel<false, MODE>, grid, BLK, stream, f, ws,
                                                f->N, A, pw.proj, pw.aux);
                }
            } else if (aux)
                launch_project_backward(frame_project_backward_adam_aux_kernel<CD, BLK, MODE>, grid, BLK, stream, f, ws, f->N, A);
            else
                launch_project_backward(frame_project_backward_kernel<CD, 0, BLK, MODE>, grid, BLK, stream, f, ws, f->N,
                                        (int64_t)0, nullptr, nullptr, nullptr, nullptr, nullptr, A);
        };
        if (nt)
            launch(gs_int<2>{});
        else
            launch(gs_int<1>{});
    });
    GS_CHECK_LAUNCH();
    return 0;
}

// Gaussians [g_begin, g_end), as gs_stage_aux_depth_backward
int gs_stage_project_backward(const gs_frame *f, const gs_frame_ws &ws, float *grad_pos, float *grad_quat,
                              float *grad_scale, float *grad_opa, float *grad_rgb, int part, int64_t g_begin,
                              int64_t g_end, hipStream_t stream) {
    if (g_end <= g_begin) return 0;
    gs_for_color_dim(f->color_dim, [&](auto cd) {
        constexpr int CD = decltype(cd)::value, BLK = CD == 3 ? 256 : 128;
        auto launch = [&](auto pt) {
            launch_project_backward(frame_project_backward_kernel<CD, decltype(pt)::value>,
                                    (unsigned)gs_div_up(g_end - g_begin, BLK), BLK, stream, f, ws, g_end, g_begin, grad_pos,
                                    (float4 *)grad_quat, grad_scale, grad_opa, grad_rgb, AdamFusedDev{});
        };
        if (part == 1)
            launch(gs_int<1>{});
        else if (part == 2)
            launch(gs_int<2>{});
        else
            launch(gs_int<0>{});
    });
    GS_CHECK_LAUNCH();
    return 0;
}
