// overlap_point.h -- the per-point decision of gs_view_overlap (include/gs_abi.h), written once for the device and the host.
//
// A frame measured a range z at lattice pixel (x, y); the surface point it saw is the one seed.hip writes for that pixel, in
// seed.hip's operation order (restated here, not shared: seed.hip's device code stays what it is).  View k sees the point
// when it lies beyond `near` in front of the view and projects inside the view's image less `border` pixels a side.  All of it
// is fp32 with one rounding per operation: every translation unit that includes this file is compiled with
// -ffp-contract=off, division and square root are correctly rounded, so the kernel, a host compilation of this text and the
// float32 restatement of tests/overlap_ref.py decide every point alike.
//   measured:  z > 0 and finite (the rule of gs_seed and gs_loss_depth)
//   point:     u = (x + left - padW / 2 + 0.5) / fx,  v likewise;  z_cam = z / sqrt(u u + v v + 1);
//              p = rot^T ((u z_cam, v z_cam, z_cam) - tran)
//   view k:    q = rot_k p + tran_k, each row summed left to right;  cx = padW_k / 2 - left_k, cy likewise (small integers);
//              seen  <=>  q.z > near  and  fl(fx_k q.x) >= fl((border - cx) q.z)  and  fl(fx_k q.x) < fl((W_k - border - cx) q.z)
//                         and the same two for y
// -- the inverse of the renderer's pixel coordinate (raster_pixel_coord), cross-multiplied: no division in the test.
// Cameras whose principal point is off the renderer's centre by (dx, dy) pixels (gs_view_overlap_pp; the *_pp functions below):
//   point:     u = fl(fl(fl((float)(x + left - padW / 2) + 0.5f) - dx) / fx),  v likewise  (the ray of gs_seed_apply_pp)
//   view k:    every bound moves by the view's own offset before it is multiplied:
//              fl(fx_k q.x) >= fl(fl((float)(border - cx) - dx_k) q.z)  and  fl(fx_k q.x) < fl(fl((float)(W_k - border - cx) - dx_k) q.z)
// The functions without the suffix are what they were: a call without offsets runs them.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gs_abi.h"

#if defined(__HIPCC__)
#define GS_OVERLAP_HD __host__ __device__
#else
#define GS_OVERLAP_HD
#endif

static_assert(sizeof(gs_seed_camera) == 64, "a view row is one 64-byte line");

// left - padW / 2 of the frame path's padded image and centred crop (splatter.py:267-272): the padded-image pixel index of
// pixel 0 minus half the padded size.  An exact small integer; minus the `cx` of the text above.
GS_OVERLAP_HD inline int32_t gs_overlap_origin(int32_t size) {
    const int32_t pad = (size + 15) / 16 * 16;
    return (pad - size) / 2 - pad / 2;
}

GS_OVERLAP_HD inline bool gs_overlap_measured(float z) { return z > 0.f && z <= FLT_MAX; }  // (false for NaN and +inf)

// the world point of lattice pixel (x, y) with range z, seen by the camera `c`
GS_OVERLAP_HD inline void gs_overlap_point(const gs_seed_camera &c, int32_t x, int32_t y, float z, float p[3]) {
    const float u = ((float)(x + gs_overlap_origin(c.width)) + 0.5f) / c.focal_x;
    const float v = ((float)(y + gs_overlap_origin(c.height)) + 0.5f) / c.focal_y;
    const float zc = z / sqrtf(u * u + v * v + 1.0f);
    const float q0 = u * zc - c.tran[0], q1 = v * zc - c.tran[1], q2 = zc - c.tran[2];
    for (int k = 0; k < 3; ++k) p[k] = c.rot[k] * q0 + c.rot[3 + k] * q1 + c.rot[6 + k] * q2;
}

// does view `w` see the world point p?
GS_OVERLAP_HD inline bool gs_overlap_seen(const float p[3], const gs_seed_camera &w, float near, int32_t border) {
    const float qx = w.rot[0] * p[0] + w.rot[1] * p[1] + w.rot[2] * p[2] + w.tran[0];
    const float qy = w.rot[3] * p[0] + w.rot[4] * p[1] + w.rot[5] * p[2] + w.tran[1];
    const float qz = w.rot[6] * p[0] + w.rot[7] * p[1] + w.rot[8] * p[2] + w.tran[2];
    const int32_t ox = gs_overlap_origin(w.width), oy = gs_overlap_origin(w.height);  // -cx, -cy
    const float fx = w.focal_x * qx, fy = w.focal_y * qy;
    // (`&` on purpose: five compares and four ANDs, no branch per condition)
    return (qz > near) & (fx >= (float)(border + ox) * qz) & (fx < (float)(w.width - border + ox) * qz)
           & (fy >= (float)(border + oy) * qz) & (fy < (float)(w.height - border + oy) * qz);
}

// ---- cameras with an off-centre principal point ((dx, dy) = c's offset in pixels)
GS_OVERLAP_HD inline void gs_overlap_point_pp(const gs_seed_camera &c, float dx, float dy, int32_t x, int32_t y, float z,
                                              float p[3]) {
    const float un = ((float)(x + gs_overlap_origin(c.width)) + 0.5f) - dx;
    const float vn = ((float)(y + gs_overlap_origin(c.height)) + 0.5f) - dy;
    const float u = un / c.focal_x, v = vn / c.focal_y;
    const float zc = z / sqrtf(u * u + v * v + 1.0f);
    const float q0 = u * zc - c.tran[0], q1 = v * zc - c.tran[1], q2 = zc - c.tran[2];
    for (int k = 0; k < 3; ++k) p[k] = c.rot[k] * q0 + c.rot[3 + k] * q1 + c.rot[6 + k] * q2;
}

GS_OVERLAP_HD inline bool gs_overlap_seen_pp(const float p[3], const gs_seed_camera &w, float dx, float dy, float near,
                                             int32_t border) {
    const float qx = w.rot[0] * p[0] + w.rot[1] * p[1] + w.rot[2] * p[2] + w.tran[0];
    const float qy = w.rot[3] * p[0] + w.rot[4] * p[1] + w.rot[5] * p[2] + w.tran[1];
    const float qz = w.rot[6] * p[0] + w.rot[7] * p[1] + w.rot[8] * p[2] + w.tran[2];
    const int32_t ox = gs_overlap_origin(w.width), oy = gs_overlap_origin(w.height);  // -cx, -cy
    const float fx = w.focal_x * qx, fy = w.focal_y * qy;
    const float x_lo = (float)(border + ox) - dx, x_hi = (float)(w.width - border + ox) - dx;
    const float y_lo = (float)(border + oy) - dy, y_hi = (float)(w.height - border + oy) - dy;
    return (qz > near) & (fx >= x_lo * qz) & (fx < x_hi * qz) & (fy >= y_lo * qz) & (fy < y_hi * qz);
}
