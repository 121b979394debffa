// project_common.h -- what the projection (cull_project.hip) and its backward (project_bwd.hip) both need: the camera
// transform and the EWA covariance projection (world2camera, gaussian.cu:49-99; jacobian, :10-47; the forward half of
// global_culling_kernel, :1182-1336), the activations, and the per-frame parameter block the kernels of both files take
// by value.  Every expression is written in the reference's source order; both files are compiled with
// -ffp-contract=off, each for its own reason (see their headers).  The forward's per-Gaussian work is stated once, in two
// halves: make_static (what depends on the Gaussian alone; a scene pack caches its result, cull_project.hip) and the camera
// half (project_cull + project_cov_static), so that a packed frame evaluates the same expressions on the same inputs in the
// same order as a raw one.
#pragma once
#include <math.h>
#include "gs_common.h"
#include "gs_frame_layout.h"

namespace {

struct Cam {
    float rot[9];
    float tran[3];
};

__device__ __forceinline__ void world_to_camera(const float p[3], const Cam &cam, float pc[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
        pc[i] = cam.rot[i * 3 + 0] * p[0] + cam.rot[i * 3 + 1] * p[1] + cam.rot[i * 3 + 2] * p[2] +
                cam.tran[i];
}

__device__ __forceinline__ void quat_to_R(float w, float x, float y, float z, float R[9]) {
    R[0] = 1 - 2 * y * y - 2 * z * z;
    R[1] = 2 * x * y - 2 * z * w;
    R[2] = 2 * x * z + 2 * y * w;
    R[3] = 2 * x * y + 2 * z * w;
    R[4] = 1 - 2 * x * x - 2 * z * z;
    R[5] = 2 * y * z - 2 * x * w;
    R[6] = 2 * x * z - 2 * y * w;
    R[7] = 2 * y * z + 2 * x * w;
    R[8] = 1 - 2 * x * x - 2 * y * y;
}

__device__ __forceinline__ void mm3(const float A[9], const float B[9], float C[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += A[r * 3 + k] * B[k * 3 + c];
            C[r * 3 + c] = s;
        }
}
__device__ __forceinline__ void mm3_nt(const float A[9], const float B[9], float C[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += A[r * 3 + k] * B[c * 3 + k];
            C[r * 3 + c] = s;
        }
}

// Rows 0,1 of J*W (row 2 of the Jacobian never reaches the 2x2 covariance).  JW is 3x3 with
// row 2 left zero so the 3x3 products below have the reference's shape; the compiler drops
// the dead row.
__device__ __forceinline__ void jacobian_rows(const float pc[3], float J[9]) {
    float u0 = pc[0], u1 = pc[1], u2 = pc[2];
    J[0] = 1 / u2;
    J[1] = 0;
    J[2] = -u0 / (u2 * u2);
    J[3] = 0;
    J[4] = 1 / u2;
    J[5] = -u1 / (u2 * u2);
    J[6] = 0;
    J[7] = 0;
    J[8] = 0;
}

// Returns false when culled.  pos_i = (x/z, y/z, |p_c|), cov = (S00, S01, S10, S11).
// `project` in two halves:
// project_cull = camera transform + near plane + frustum test -> pc, pos_i[0..1]; project_cov = depth + covariance.
__device__ __forceinline__ bool project_cull(const float p[3], const Cam &cam, float near_plane, float half_w,
                                             float half_h, float pc[3], float pos_i[3]) {
    world_to_camera(p, cam, pc);
    if (pc[2] <= near_plane) return false;
    pos_i[0] = pc[0] / pc[2];
    pos_i[1] = pc[1] / pc[2];
    return !(fabsf(pos_i[0]) >= half_w || fabsf(pos_i[1]) >= half_h);
}
// project_cov in two halves: static_cov = what depends on the Gaussian alone (R S S R^T), project_cov_static = depth + what the
// camera adds.  Each half is the reference's expressions in the reference's order: the halves share no intermediate.
__device__ __forceinline__ void static_cov(const float q[4], const float s[3], float RSSR[9]) {
    float R[9], S[9] = {s[0], 0, 0, 0, s[1], 0, 0, 0, s[2]}, RS[9];
    quat_to_R(q[0], q[1], q[2], q[3], R);
    mm3(R, S, RS);
    mm3_nt(RS, RS, RSSR);
}
__device__ __forceinline__ void project_cov_static(const float pc[3], const float RSSR[9], const Cam &cam, float pos_i[3],
                                                   float cov[4]) {
    pos_i[2] = sqrtf(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
    float J[9], JW[9], JWC[9], JWCWJ[9];
    jacobian_rows(pc, J);
    mm3(J, cam.rot, JW);
    mm3(JW, RSSR, JWC);
    mm3_nt(JWC, JW, JWCWJ);
    cov[0] = JWCWJ[0];
    cov[1] = JWCWJ[1];
    cov[2] = JWCWJ[3];
    cov[3] = JWCWJ[4];
}
__device__ __forceinline__ void project_cov(const float pc[3], const float q[4], const float s[3], const Cam &cam,
                                            float pos_i[3], float cov[4]) {
    float RSSR[9];
    static_cov(q, s, RSSR);
    project_cov_static(pc, RSSR, cam, pos_i, cov);
}
__device__ __forceinline__ bool project(const float p[3], const float q[4], const float s[3],
                                        const Cam &cam, float near_plane, float half_w, float half_h,
                                        float pos_i[3], float cov[4]) {
    float pc[3];
    if (!project_cull(p, cam, near_plane, half_w, half_h, pc, pos_i)) return false;
    project_cov(pc, q, s, cam, pos_i, cov);
    return true;
}

__device__ __forceinline__ void load3(const float *base, int64_t i, float v[3]) {
    v[0] = base[i * 3 + 0];
    v[1] = base[i * 3 + 1];
    v[2] = base[i * 3 + 2];
}

// The per-frame parameters of the projection and of its backward (make_params below), passed to the kernels by value.
struct ProjectParams {
    Cam cam;
    float near_plane, half_w, half_h;
    float tlog;  // -2*logf(thresh), computed on the host
    float tlx, tly, leftmost, topmost;
    uint32_t ntx, nty;
    int32_t scale_act;
    int32_t color_dim;
    int32_t cull_method;        // 0: "dist" (tile centres), 1: "prob" (tile edges), 2: "prob2" (index arithmetic)
    float dist_thresh, dist_radius;  // "dist": squared distance threshold (splatter.py:577) and its square root
    float half_padw, half_padh;  // padded size / 2, in pixels (exact in fp32)
    float fx, fy;
    // occlusion test of frame_project_cull_count_kernel (conservative, never compared bit for bit): 1 / tlx, 1 / tly and
    // 1.02 x sqrt(tlog) x the largest singular value of the camera rotation (1 for a rotation; the caller's matrix is not trusted)
    float inv_tlx, inv_tly, occ_k;
    // GS_FRAME_PRINCIPAL_POINT: the principal point's offset from the renderer's centre, over the focal lengths (make_params,
    // in double, rounded once); pp = 0: a centred frame, which runs the kernels without the addition -- the PP = false
    // instantiations below, the kernels from before the flag existed (an unconditional + 0.0f would turn a stored -0 into +0)
    float sx, sy;
    int32_t pp;
};

// project_cull of the frame path: the same camera transform, near plane and frustum test; PP: the principal point's offset is
// added to the projected centre -- pos_i = (fl(fl(x / z) + sx), fl(fl(y / z) + sy)) -- BEFORE the frustum test (the guard band
// stays centred on the image).  Everything downstream reads this centre; J, the covariance and every backward are functions
// of p_c alone and do not see the offset (a constant added to pos_i has derivative 1).  A compile-time variant: the project
// kernels of a flagged frame are instantiations of their own (cull_project.hip, *_pp_kernel).
template <bool PP>
__device__ __forceinline__ bool project_cull(const float p[3], const ProjectParams &P, float pc[3], float pos_i[3]) {
    world_to_camera(p, P.cam, pc);
    if (pc[2] <= P.near_plane) return false;
    pos_i[0] = pc[0] / pc[2];
    pos_i[1] = pc[1] / pc[2];
    if (PP) {
        pos_i[0] = pos_i[0] + P.sx;
        pos_i[1] = pos_i[1] + P.sy;
    }
    return !(fabsf(pos_i[0]) >= P.half_w || fabsf(pos_i[1]) >= P.half_h);
}

// sigmoid on the transcendental unit (v_exp_f32 + v_rcp_f32, ~2 ulp): the opacity / colour activations feed the
// compositing only (image tolerance 5e-5), not the integer side of the pipeline; expf + an IEEE division cost
// ~25 instructions each, four times per Gaussian, in a kernel that is VALU-issue bound
__device__ __forceinline__ float sigmoid_f(float x) { return gs_rcp(1.0f + gs_exp2(-GS_LOG2E * x)); }

__device__ __forceinline__ void activate(const float qraw[4], const float sraw[3], int scale_act,
                                         float q[4], float s[3]) {
    float nr = sqrtf(qraw[0] * qraw[0] + qraw[1] * qraw[1] + qraw[2] * qraw[2] + qraw[3] * qraw[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qraw[k] / nr;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = scale_act == 0 ? fabsf(sraw[k]) + 1e-4f : expf(sraw[k]);
}

// Raw parameters of one Gaussian (what S1 reads: 56 bytes with rgb logits, 44 with SH)
struct RawGaussian {
    float p[3], sraw[3], qraw[4], opa, rgb[3];
};
// The camera-independent half of S1 for one Gaussian: position, R S S R^T (all nine entries), the activated opacity and
// the rgb colour (zero with SH colours, which the compositing evaluates per pixel).  It is what a scene pack stores
// (cull_project.hip): the camera half below it takes this and nothing else of the Gaussian.
struct StaticGaussian {
    float p[3], RSSR[9], opa_act, col[3];
};
// `s`: the activated scales as well (the scene pack keeps the largest)
__device__ __forceinline__ StaticGaussian make_static(const RawGaussian &in, int scale_act, int color_dim, float s[3]) {
    StaticGaussian g;
    float q[4];
    activate(in.qraw, in.sraw, scale_act, q, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) g.p[k] = in.p[k];
    static_cov(q, s, g.RSSR);
    g.opa_act = sigmoid_f(in.opa);
    g.col[0] = g.col[1] = g.col[2] = 0.f;
    if (color_dim == 3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g.col[k] = sigmoid_f(in.rgb[k]);
    }
    return g;
}
__device__ __forceinline__ StaticGaussian make_static(const RawGaussian &in, int scale_act, int color_dim) {
    float s[3];
    return make_static(in, scale_act, color_dim, s);
}

// Grid of the grid-stride reference-API kernels (section A of both files)
inline int grid_for(int64_t n, int block) {
    int64_t g = gs_div_up(n, block);
    if (g > 8192) g = 8192;  // 256 CUs x 8 blocks x 4: grid-stride beyond that
    if (g < 1) g = 1;
    return (int)g;
}

inline ProjectParams make_params(const gs_frame *f) {
    ProjectParams P;
    for (int i = 0; i < 9; ++i) P.cam.rot[i] = f->rot[i];
    for (int i = 0; i < 3; ++i) P.cam.tran[i] = f->tran[i];
    P.near_plane = f->near_plane;
    P.half_w = f->half_width;
    P.half_h = f->half_height;
    P.tlog = -2 * logf(f->thresh);
    P.dist_thresh = f->thresh;
    P.dist_radius = sqrtf(f->thresh);
    gs_frame_geom G = gs_frame_geometry(f);
    P.tlx = G.tlx;
    P.tly = G.tly;
    P.leftmost = G.leftmost;
    P.topmost = G.topmost;
    P.ntx = (uint32_t)G.ntx;
    P.nty = (uint32_t)G.nty;
    P.scale_act = f->scale_activation;
    P.color_dim = f->color_dim;
    P.cull_method = f->tile_culling_method;
    P.half_padw = (float)(G.padW / 2);
    P.half_padh = (float)(G.padH / 2);
    P.fx = f->focal_x;
    P.fy = f->focal_y;
    P.sx = P.sy = 0.f;
    P.pp = 0;
    if (f->flags & GS_FRAME_PRINCIPAL_POINT) {
        const gs_frame_pp *e = gs_frame_pp_fields(f);
        P.sx = (float)(e->pp_dx / (double)f->focal_x);
        P.sy = (float)(e->pp_dy / (double)f->focal_y);
        P.pp = (e->pp_dx != 0.0 || e->pp_dy != 0.0) ? 1 : 0;  // a zero offset is no offset
    }
    P.inv_tlx = 1.0f / G.tlx;
    P.inv_tly = 1.0f / G.tly;
    {   // largest singular value of the camera rotation as given (power iteration on W^T W; 1 for a rotation)
        double A[9], v[3] = {0.6, 0.5, 0.62}, lam = 1.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                A[i * 3 + j] = 0;
                for (int k = 0; k < 3; ++k) A[i * 3 + j] += (double)f->rot[k * 3 + i] * (double)f->rot[k * 3 + j];
            }
        for (int it = 0; it < 48; ++it) {
            double w[3];
            for (int i = 0; i < 3; ++i) w[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
            lam = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            if (!(lam > 0)) break;
            for (int i = 0; i < 3; ++i) v[i] = w[i] / lam;
        }
        // (power iteration approaches the largest eigenvalue from below: 1 % on top; trace as the fail-safe upper bound)
        const double tr = A[0] + A[4] + A[8];
        double sig = sqrt(lam) * 1.01;
        if (!(sig > 0) || !(sig <= sqrt(tr) * 1.01)) sig = sqrt(tr) * 1.01;
        P.occ_k = (float)(1.02 * sqrt((double)P.tlog) * sig);
    }
    return P;
}

}  // namespace
