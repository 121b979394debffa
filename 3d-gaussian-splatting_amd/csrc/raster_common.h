// raster_common.h -- shared pieces of the tile rasterizer forward/backward kernels.
#pragma once
// SH colours sigma(sum_k sh_k(pixel) coef_k) are evaluated as 1 / (1 + 2^(sum_k sh'_k coef_k)) with the pixel's basis
// values pre-scaled once per wave, sh'_k = -log2(e) sh_k: the exponential's argument needs no multiplication per
// (pixel, Gaussian, channel) -- 12 VALU instructions per Gaussian step of a wave in the SH forward and backward
// kernels (8 % of the forward's).
#include "gs_common.h"
#include "gs_frame_layout.h"

// Where the Gaussians of a tile's sorted list live.
//  FRAME = true : sorted Gaussian ids + N-indexed records written by stage S1 (no sorted
//                 attribute copies exist; gathers hit L2 / Infinity Cache).
//  FRAME = false: the reference API -- attributes already gathered in sorted order
//                 (pos[M,3], rgb[M,D], opa[M], cov[M,2,2]; gaussian.cu:806-813).
struct RasterSrc {
    const uint32_t *ids;
    const float4 *geom;    // (x, y, depth, opacity)   } interleaved, stride GS_REC_STRIDE float4
    const float4 *cov4;    // (a, b, c, d)             } (one 64-byte record per Gaussian)
    const float4 *color4;  // (r, g, b, -)             }
    const float4 *conic4;  // (A, B, C, -)             }
    const float *sh;       // raw rgb parameter [N,27 | 48] (SH coefficients, channel-major)
    const float *pos, *rgb, *opa, *cov;
};

struct RasterGeom {
    int32_t padW, padH, ntx, nty;
    int32_t width, height, crop_top, crop_left;  // un-padded output (frame path)
    float focal_x, focal_y;
    float rays_o[3], lefttop[3], vdx[3], vdy[3];
    // reference API (gs_draw / gs_draw_backward): the ray basis arrives as four DEVICE tensors of three floats; the
    // kernels read them themselves (uniform loads in the prologue) instead of the host copying them back and
    // synchronising the stream.  All NULL on the frame path, which passes the basis by value above.
    const float *dev_rays_o, *dev_lefttop, *dev_vdx, *dev_vdy;
};

// The (S, G) of a frame-path launch, forward or backward: the frame's records under the sorted ids, its padded and cropped
// geometry and its ray basis by value.
static inline void gs_frame_raster_args(const gs_frame *f, const gs_frame_ws &ws, const uint32_t *sorted_ids, RasterSrc &S,
                                        RasterGeom &G) {
    const gs_frame_geom FG = gs_frame_geometry(f);
    S = {};
    S.ids = sorted_ids;
    S.geom = ws.rec_geom;
    S.cov4 = ws.rec_cov;
    S.color4 = ws.rec_color;
    S.conic4 = ws.rec_conic;
    S.sh = f->rgb;
    G = {};
    G.padW = FG.padW;
    G.padH = FG.padH;
    G.ntx = FG.ntx;
    G.nty = FG.nty;
    G.width = f->width;
    G.height = f->height;
    G.crop_top = FG.crop_top;
    G.crop_left = FG.crop_left;
    G.focal_x = f->focal_x;
    G.focal_y = f->focal_y;
    for (int i = 0; i < 3; ++i) {
        G.rays_o[i] = f->rays_o[i];
        G.lefttop[i] = f->lefttop[i];
        G.vdx[i] = f->vec_dx[i];
        G.vdy[i] = f->vec_dy[i];
    }
}
// The (S, G) of a reference-API call (gs_draw / gs_draw_backward, raster_fwd_ref.hip): attributes in sorted order, whole tiles,
// and with SH colours the ray basis.  Nonzero: refused (SH without the basis), the error set under the name `entry`.
int gs_ref_raster_args(const char *entry, const float *pos, const float *rgb, const float *opa, const float *cov, int32_t h,
                       int32_t w, float focal_x, float focal_y, int use_sh_coeff, const float *rays_o,
                       const float *lefttop_pos, const float *vec_dx, const float *vec_dy, RasterSrc &S, RasterGeom &G);
// The reference API's forward (raster_fwd_ref.hip); gs_draw_backward replays it for the checkpoints (`ckpt` != NULL).  `exact`:
// the reference's `fast = 0` flavour of the exponential (double division + double exp per pixel, gaussian.cu:922-923).
int gs_raster_forward_ref(const RasterSrc &S, const RasterGeom &G, const int32_t *accum, float *res, int use_sh,
                          int sigmoid, int weight_normalize, float4 *ckpt, uint32_t *tile_nproc,
                          hipStream_t stream, int exact);

struct GaussianRec {
    float x, y, a, b, c, d, opa;
};

template <bool FRAME>
__device__ __forceinline__ uint32_t raster_load(const RasterSrc &S, uint32_t j, GaussianRec &g) {
    if (FRAME) {
        const uint32_t id = S.ids[j];
        const float4 ge = S.geom[(size_t)id * GS_REC_STRIDE], cv = S.cov4[(size_t)id * GS_REC_STRIDE];
        g.x = ge.x;
        g.y = ge.y;
        g.opa = ge.w;
        g.a = cv.x;
        g.b = cv.y;
        g.c = cv.z;
        g.d = cv.w;
        return id;
    } else {
        g.x = S.pos[(size_t)j * 3 + 0];
        g.y = S.pos[(size_t)j * 3 + 1];
        g.opa = S.opa[j];
        const float4 cv = reinterpret_cast<const float4 *>(S.cov)[j];
        g.a = cv.x;
        g.b = cv.y;
        g.c = cv.z;
        g.d = cv.w;
        return j;
    }
}

template <bool FRAME>
__device__ __forceinline__ void raster_load_rgb(const RasterSrc &S, uint32_t j, uint32_t id, float &r, float &g,
                                                float &b) {
    if (FRAME) {
        const float4 c = S.color4[(size_t)id * GS_REC_STRIDE];
        r = c.x;
        g = c.y;
        b = c.z;
    } else {
        r = S.rgb[(size_t)j * 3 + 0];
        g = S.rgb[(size_t)j * 3 + 1];
        b = S.rgb[(size_t)j * 3 + 2];
    }
}

template <bool FRAME, int CDIM>
__device__ __forceinline__ const float *raster_sh_ptr(const RasterSrc &S, uint32_t j, uint32_t id) {
    return FRAME ? S.sh + (size_t)id * CDIM : S.rgb + (size_t)j * CDIM;
}

__device__ __forceinline__ float raster_det(float a, float b, float c, float d) { return gs_det(a, b, c, d); }
__device__ __forceinline__ void raster_conic(const GaussianRec &g, float &A, float &B, float &C) {
    gs_conic(g.a, g.b, g.c, g.d, A, B, C);
}

// Pixel centre in normalised image units.  The reference evaluates (id + 0.5 - w/2) / focal in double
// and rounds to float (gaussian.cu:839-840).  The numerator is a half-integer (exact in fp32), so one
// correctly-rounded fp32 division gives the same float except in the ~2^-29 of cases where the double
// quotient sits within half a double-ulp of an fp32 rounding boundary (then 1 ulp): two fp64 divisions
// per lane were ~15 % of this kernel's per-tile prologue.
__device__ __forceinline__ float raster_pixel_coord(uint32_t id, int32_t padded, float focal) {
    return ((float)id + 0.5f - (float)((uint32_t)padded / 2)) / focal;
}

// Per-pixel SH basis (gaussian.cu:849-861, 405-426), same promotions as the reference.  NB = 9 is the reference's
// degree 2.  NB = 16 adds the degree-3 band in the same (svox2) sign convention with the C3 table the reference
// declares (gaussian.cu:395-403) but never reads -- BASELINE config 4 names "SH degree 3"; it is an extension.
template <int NB>
__device__ __forceinline__ void raster_pixel_sh(uint32_t id_x, uint32_t id_y, const RasterGeom &G, float *SH) {
    float dir[3], nrm = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const bool dev = G.dev_rays_o != nullptr;  // uniform
        const float lt = dev ? G.dev_lefttop[i] : G.lefttop[i], vx = dev ? G.dev_vdx[i] : G.vdx[i];
        const float vy = dev ? G.dev_vdy[i] : G.vdy[i], ro = dev ? G.dev_rays_o[i] : G.rays_o[i];
        dir[i] = lt + id_x * vx + id_y * vy - ro;
        nrm += dir[i] * dir[i];
    }
    nrm = sqrtf(nrm);
#pragma unroll
    for (int i = 0; i < 3; ++i) dir[i] = (float)(dir[i] / (nrm + 1e-7));
    const float x = dir[0], y = dir[1], z = dir[2];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    SH[0] = 0.28209479177387814f;
    SH[1] = -0.4886025119029199f * y;
    SH[2] = 0.4886025119029199f * z;
    SH[3] = -0.4886025119029199f * x;
    SH[4] = 1.0925484305920792f * xy;
    SH[5] = -1.0925484305920792f * yz;
    SH[6] = (float)(0.31539156525252005f * (2.0 * zz - xx - yy));
    SH[7] = -1.0925484305920792f * xz;
    SH[8] = 0.5462742152960396f * (xx - yy);
    if (NB == 16) {
        SH[9] = -0.5900435899266435f * y * (3.0f * xx - yy);
        SH[10] = 2.890611442640554f * xy * z;
        SH[11] = -0.4570457994644658f * y * (4.0f * zz - xx - yy);
        SH[12] = 0.3731763325901154f * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        SH[13] = -0.4570457994644658f * x * (4.0f * zz - xx - yy);
        SH[14] = 1.445305721320277f * z * (xx - yy);
        SH[15] = -0.5900435899266435f * x * (xx - 3.0f * yy);
    }
}

// Checkpoint slot of local bucket b of a tile whose sorted list starts at `start`:
// floor(start/64) + tile + b.  Slots of different tiles never overlap and the total is
// <= M/64 + T, so no scan is needed before the forward pass.
__device__ __forceinline__ size_t raster_ckpt_slot(uint32_t start, uint32_t tile, uint32_t b) {
    return (size_t)(start / GS_BUCKET) + tile + b;
}

// The DPP row scans of the row-layout kernels, for the lane's four pixels at once and every step ONE instruction per pixel
// (v_mul_f32_dpp v, v, v row_shr:n: lanes whose source falls outside the row are disabled by the DPP bound check and keep v --
// the identity for free; through the builtin the compiler emits v_mov 1.0 + v_mov_dpp + v_mul for a product step).  The four
// chains are interleaved so that the write of a register and its DPP read in the next step are three instructions apart (the
// hardware wants two wait states there, and the compiler's hazard pass does not look into inline assembly: hence also the
// s_nop in front of a block).
//
// Inclusive prefix sum over the 16 lanes of a DPP row for the lane's four pixels, OUT of place: the first step's
// bound_ctrl:0 reads 0 where a lane has no source -- the sum's identity --, so `in` survives (round 5: the unscanned w gc
// gives s = w gc - rho beta one instruction cheaper than dL/dalpha alpha).
__device__ __forceinline__ void gs_row_scan_add4_oop(float out[4], const float in[4]) {
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %4, %4 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %1, %5, %5 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %2, %6, %6 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %3, %7, %7 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %1, %1, %1 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %2, %2, %2 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %3, %3, %3 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %1, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %2, %2, %2 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %3, %3, %3 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %1, %1, %1 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %2, %2, %2 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_add_f32_dpp %3, %3, %3 row_shr:8 row_mask:0xf bank_mask:0xf"
                 : "=&v"(out[0]), "=&v"(out[1]), "=&v"(out[2]), "=&v"(out[3])
                 : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]));
    // (no s_nop behind the block: the hazard is VALU write -> DPP READ; what follows reads the results with plain VALU
    // instructions, and the kernels that use this helper contain no compiler-generated DPP instruction)
}
// Both at once (one asm block, no s_nop between the two: a register written by the scan's last step is read four
// instructions later): p <- inclusive product scan of p; t <- t x (scanned p of the lane to the left), lane 0 keeps t.
__device__ __forceinline__ void gs_row_scan_mul4_excl(float p[4], float t[4]) {
    asm volatile("s_nop 1\n\t"
                 "v_mul_f32_dpp %4, %4, %4 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %5, %5, %5 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %6, %6, %6 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %7, %7, %7 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %4, %4, %4 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %5, %5, %5 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %6, %6, %6 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %7, %7, %7 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %4, %4, %4 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %5, %5, %5 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %6, %6, %6 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %7, %7, %7 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %4, %4, %4 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %5, %5, %5 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %6, %6, %6 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %7, %7, %7 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %0, %4, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %1, %5, %1 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %2, %6, %2 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %3, %7, %3 row_shr:1 row_mask:0xf bank_mask:0xf"
                 : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]));
}
