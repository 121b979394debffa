// icp_point.h -- the per-pixel arithmetic of gs_icp_model_maps and gs_icp_step (include/gs_abi.h), written once for the device
// and the host.
//
// Point-to-plane ICP of an incoming range map against the map's own vertex / normal maps.  Everything here is fp32 with one
// rounding per operation: every translation unit that includes this file is compiled with -ffp-contract=off, division and
// square root are correctly rounded, so the kernels, a host compilation of this text and the float32 restatement of
// tests/icp_ref.py compute every vertex, every normal and every keep / drop decision alike.  The ray is the one of
// gs_overlap_point_pp (overlap_point.h), restated here, not shared: the device code of seed.hip and overlap.hip stays what it is.
//   measured:  z > 0 and finite (gs_overlap_measured's rule)
//   ray:       u = fl(fl(fl((float)(x + left - padW / 2) + 0.5f) - dx) / fx),  v likewise;  s = sqrtf(u u + v v + 1)
//              (offsets (0, 0): the bits of the centred ray -- x - 0.0f is x)
//   point:     zc = z / s;  p = (u zc, v zc, zc)  -- the range z along the unit ray, in the camera's frame
//   model:     rho = D / A where A >= alpha_min (alpha given), else D;  vertex = point(rho), w = 1 where rho is measured
//   normal:    a = v[x+s] - v[x-s],  b = v[y+s] - v[y-s],  c = a x b,  l = sqrtf(c.c);  n = c / l, negated where n.v > 0;
//              valid where the five pixels are inside the image and measured, hi <= fl(fl(1 + edge_rel) lo) over their ranges
//              (edge_rel < 0: no edge test) and l > 0 and finite
//   step:      q = R p + t, each row summed left to right, R and t the state rounded to fp32 once
//              model pixel: f = fl(fl(fl(fx_m fl(q.x / q.z)) + dx_m) - (float)(left_m - padW_m / 2)),  i = floor(f), pixel i
//              covers [i, i + 1) -- the inverse of the renderer's pixel coordinate (raster_pixel_coord); j likewise
//              kept  <=>  q.z > 0  and  0 <= f < W_m (and y)  and  the normal at (i, j) is valid
//                         and  |q - v|^2 <= fl(dist_max dist_max)  and  -(n.v) >= fl(cos_min sqrtf(v.v))
//              e = n.(q - v),  J = (q x n, n);  28 terms: J_i J_j (i <= j, row-major), J_i e, e e
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_abi.h"

#if defined(__HIPCC__)
#define GS_ICP_HD __host__ __device__
#else
#define GS_ICP_HD
#endif

#define GS_ICP_TERMS 28  // 21 of J J^T, 6 of J e, e e

// a camera as the ICP kernels read it: no pose (the maps live in the camera's own frame)
struct gs_icp_cam {
    float fx, fy, dx, dy;
    int32_t W, H, ox, oy;  // ox = left - padW / 2 of the frame path's padded image (gs_icp_origin), oy likewise
};

GS_ICP_HD inline int32_t gs_icp_origin(int32_t size) {
    const int32_t pad = (size + 15) / 16 * 16;
    return (pad - size) / 2 - pad / 2;
}

GS_ICP_HD inline gs_icp_cam gs_icp_camera(const gs_seed_camera_pp &c) {
    gs_icp_cam k;
    k.fx = c.cam.focal_x, k.fy = c.cam.focal_y, k.dx = c.pp_dx, k.dy = c.pp_dy;
    k.W = c.cam.width, k.H = c.cam.height;
    k.ox = gs_icp_origin(c.cam.width), k.oy = gs_icp_origin(c.cam.height);
    return k;
}

GS_ICP_HD inline bool gs_icp_measured(float z) { return z > 0.f && z <= FLT_MAX; }  // (false for NaN and +inf)

// the point at range z along the unit ray of pixel (x, y)'s centre, in the camera's frame
GS_ICP_HD inline void gs_icp_point(const gs_icp_cam &c, int32_t x, int32_t y, float z, float p[3]) {
    const float un = ((float)(x + c.ox) + 0.5f) - c.dx;
    const float vn = ((float)(y + c.oy) + 0.5f) - c.dy;
    const float u = un / c.fx, v = vn / c.fy;
    const float zc = z / sqrtf(u * u + v * v + 1.0f);
    p[0] = u * zc, p[1] = v * zc, p[2] = zc;
}

// the model's range at a pixel: D / A inside the silhouette (alpha given), the plain map otherwise; 0 = no measurement
GS_ICP_HD inline float gs_icp_model_range(const float *depth, const float *alpha, int64_t i, float alpha_min) {
    float rho = depth[i];
    if (alpha) {
        const float a = alpha[i];
        rho = a >= alpha_min ? rho / a : 0.f;
    }
    return gs_icp_measured(rho) ? rho : 0.f;
}

// vertex (x, y, z, w) and normal (x, y, z, w) of model pixel (x, y); one_plus = fl(1 + edge_rel)
GS_ICP_HD inline void gs_icp_model_pixel(const float *depth, const float *alpha, const gs_icp_cam &c, int32_t x, int32_t y,
                                         float alpha_min, float edge_rel, float one_plus, int32_t s, float vert[4],
                                         float nrm[4]) {
    vert[0] = vert[1] = vert[2] = vert[3] = 0.f;
    nrm[0] = nrm[1] = nrm[2] = nrm[3] = 0.f;
    const int64_t W = c.W, at = (int64_t)y * W + x;
    const float rho = gs_icp_model_range(depth, alpha, at, alpha_min);
    if (rho == 0.f) return;
    float v[3];
    gs_icp_point(c, x, y, rho, v);
    vert[0] = v[0], vert[1] = v[1], vert[2] = v[2], vert[3] = 1.f;
    if (!(x >= s && x < c.W - s && y >= s && y < c.H - s)) return;  // (s >= 1; W - s cannot overflow)
    const float rxp = gs_icp_model_range(depth, alpha, at + s, alpha_min), rxm = gs_icp_model_range(depth, alpha, at - s, alpha_min);
    const float ryp = gs_icp_model_range(depth, alpha, at + (int64_t)s * W, alpha_min);
    const float rym = gs_icp_model_range(depth, alpha, at - (int64_t)s * W, alpha_min);
    if (rxp == 0.f || rxm == 0.f || ryp == 0.f || rym == 0.f) return;
    const float lo = fminf(fminf(fminf(fminf(rho, rxp), rxm), ryp), rym);
    const float hi = fmaxf(fmaxf(fmaxf(fmaxf(rho, rxp), rxm), ryp), rym);
    if (!(edge_rel < 0.f || hi <= one_plus * lo)) return;
    float xp[3], xm[3], yp[3], ym[3];
    gs_icp_point(c, x + s, y, rxp, xp);
    gs_icp_point(c, x - s, y, rxm, xm);
    gs_icp_point(c, x, y + s, ryp, yp);
    gs_icp_point(c, x, y - s, rym, ym);
    const float a0 = xp[0] - xm[0], a1 = xp[1] - xm[1], a2 = xp[2] - xm[2];
    const float b0 = yp[0] - ym[0], b1 = yp[1] - ym[1], b2 = yp[2] - ym[2];
    const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const float l = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
    if (!(l > 0.f && l <= FLT_MAX)) return;
    float n0 = c0 / l, n1 = c1 / l, n2 = c2 / l;
    if (n0 * v[0] + n1 * v[1] + n2 * v[2] > 0.f) n0 = -n0, n1 = -n1, n2 = -n2;
    nrm[0] = n0, nrm[1] = n1, nrm[2] = n2, nrm[3] = 1.f;
}

// the frame point p moved into the model's frame; Rt = (R row-major, t) in fp32
GS_ICP_HD inline void gs_icp_transform(const float Rt[12], const float p[3], float q[3]) {
    q[0] = Rt[0] * p[0] + Rt[1] * p[1] + Rt[2] * p[2] + Rt[9];
    q[1] = Rt[3] * p[0] + Rt[4] * p[1] + Rt[5] * p[2] + Rt[10];
    q[2] = Rt[6] * p[0] + Rt[7] * p[1] + Rt[8] * p[2] + Rt[11];
}

// the model pixel q falls on -> its index, or -1 when q lies behind the camera or outside the image
GS_ICP_HD inline int64_t gs_icp_project(const gs_icp_cam &m, const float q[3]) {
    if (!(q[2] > 0.f)) return -1;
    const float fx = ((m.fx * (q[0] / q[2])) + m.dx) - (float)m.ox;
    const float fy = ((m.fy * (q[1] / q[2])) + m.dy) - (float)m.oy;
    if (!(fx >= 0.f && fx < (float)m.W && fy >= 0.f && fy < (float)m.H)) return -1;  // (false for NaN)
    return (int64_t)(int32_t)floorf(fy) * m.W + (int32_t)floorf(fx);
}

// the association tests behind the projection and, for a kept pixel, its 28 terms
GS_ICP_HD inline bool gs_icp_terms(const float q[3], const float v[4], const float n[4], float dist_max, float cos_min,
                                   float term[GS_ICP_TERMS]) {
    if (!(n[3] != 0.f)) return false;
    const float d0 = q[0] - v[0], d1 = q[1] - v[1], d2 = q[2] - v[2];
    if (!(d0 * d0 + d1 * d1 + d2 * d2 <= dist_max * dist_max)) return false;
    const float nv = n[0] * v[0] + n[1] * v[1] + n[2] * v[2];
    if (!(-nv >= cos_min * sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))) return false;
    const float e = n[0] * d0 + n[1] * d1 + n[2] * d2;
    float J[6];
    J[0] = q[1] * n[2] - q[2] * n[1];
    J[1] = q[2] * n[0] - q[0] * n[2];
    J[2] = q[0] * n[1] - q[1] * n[0];
    J[3] = n[0], J[4] = n[1], J[5] = n[2];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) term[k++] = J[i] * J[j];
    for (int i = 0; i < 6; ++i) term[k++] = J[i] * e;
    term[k] = e * e;
    return true;
}
