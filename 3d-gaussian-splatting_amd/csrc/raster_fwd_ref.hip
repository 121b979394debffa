// raster_fwd_ref.hip -- forward compositing behind the reference API: gs_draw, and the forward that gs_draw_backward replays.
//
// The kernel is raster_fwd_body.h's with FRAME = false: attributes in sorted order, rgb or degree-2 SH colours, with or
// without checkpoints, and the reference's sigmoid, weight_normalize and `fast = 0` flavours.
#include "raster_fwd_body.h"

// Shared with raster_bwd.hip (replay of the forward for the reference-API backward).  `exact`: the reference's
// `fast = 0` flavour of the exponential (double division + double exp per pixel, gaussian.cu:922-923).
template <int CDIM, bool CKPT>
static void fwd_ref_dispatch(const RasterSrc &S, const RasterGeom &G, const int32_t *accum, float *res, int sigmoid,
                             int weight_normalize, int exact, float4 *ckpt, uint32_t *tile_nproc, hipStream_t stream) {
    if (sigmoid) {
        if (exact)
            launch_fwd<CDIM, false, CKPT, true, true>(S, G, accum, res, nullptr, ckpt, tile_nproc, weight_normalize, stream);
        else
            launch_fwd<CDIM, false, CKPT, true, false>(S, G, accum, res, nullptr, ckpt, tile_nproc, weight_normalize, stream);
    } else {
        if (exact)
            launch_fwd<CDIM, false, CKPT, false, true>(S, G, accum, res, nullptr, ckpt, tile_nproc, weight_normalize, stream);
        else
            launch_fwd<CDIM, false, CKPT, false, false>(S, G, accum, res, nullptr, ckpt, tile_nproc, weight_normalize, stream);
    }
}
int gs_raster_forward_ref(const RasterSrc &S, const RasterGeom &G, const int32_t *accum, float *res, int use_sh,
                          int sigmoid, int weight_normalize, float4 *ckpt, uint32_t *tile_nproc,
                          hipStream_t stream, int exact) {
    if (ckpt) {
        if (use_sh)
            fwd_ref_dispatch<27, true>(S, G, accum, res, sigmoid, weight_normalize, exact, ckpt, tile_nproc, stream);
        else
            fwd_ref_dispatch<3, true>(S, G, accum, res, sigmoid, weight_normalize, exact, ckpt, tile_nproc, stream);
    } else {
        if (use_sh)
            fwd_ref_dispatch<27, false>(S, G, accum, res, sigmoid, weight_normalize, exact, nullptr, nullptr, stream);
        else
            fwd_ref_dispatch<3, false>(S, G, accum, res, sigmoid, weight_normalize, exact, nullptr, nullptr, stream);
    }
    return 0;
}

int gs_ref_raster_args(const char *entry, const float *pos, const float *rgb, const float *opa, const float *cov, int32_t h,
                       int32_t w, float focal_x, float focal_y, int use_sh_coeff, const float *rays_o,
                       const float *lefttop_pos, const float *vec_dx, const float *vec_dy, RasterSrc &S, RasterGeom &G) {
    S = {};
    S.pos = pos;
    S.rgb = rgb;
    S.opa = opa;
    S.cov = cov;
    G = {};
    G.padW = w;
    G.padH = h;
    G.ntx = w / 16;
    G.nty = h / 16;
    G.focal_x = focal_x;
    G.focal_y = focal_y;
    if (use_sh_coeff) {
        if (!(rays_o && lefttop_pos && vec_dx && vec_dy)) {
            gs_set_error("%s: invalid argument: %s", entry, "SH needs the ray basis");
            return GS_E_INVALID;
        }
        // the basis stays on the device: the kernels load it (raster_common.h), the call never synchronises
        G.dev_rays_o = rays_o;
        G.dev_lefttop = lefttop_pos;
        G.dev_vdx = vec_dx;
        G.dev_vdy = vec_dy;
    }
    return 0;
}

extern "C" int gs_draw(const float *pos, const float *rgb, const float *opa, const float *cov,
                       const int32_t *tile_n_point_accum, float *res, int32_t h, int32_t w, int64_t M,
                       float focal_x, float focal_y, int weight_normalize, int sigmoid, int fast,
                       const float *rays_o, const float *lefttop_pos, const float *vec_dx, const float *vec_dy,
                       int use_sh_coeff, gs_stream_t stream) {
    // fast != 0: v_exp_f32 on the hoisted conic (the reference's __expf); fast == 0: the exact flavour
    GS_CHECK_ARG(h > 0 && w > 0 && (h % 16) == 0 && (w % 16) == 0, "h, w must be positive multiples of 16");
    GS_CHECK_ARG(M >= 0, "M < 0");
    GS_CHECK_ARG(tile_n_point_accum && res, "null pointer");
    GS_CHECK_ARG(M == 0 || (pos && rgb && opa && cov), "null pointer");
    GS_CHECK_ARG(((uintptr_t)cov & 15) == 0, "cov must be 16-byte aligned");
    RasterSrc S;
    RasterGeom G;
    int rc = gs_ref_raster_args(__func__, pos, rgb, opa, cov, h, w, focal_x, focal_y, use_sh_coeff, rays_o, lefttop_pos, vec_dx,
                                vec_dy, S, G);
    if (rc) return rc;
    rc = gs_raster_forward_ref(S, G, tile_n_point_accum, res, use_sh_coeff, sigmoid, weight_normalize, nullptr, nullptr,
                               (hipStream_t)stream, fast ? 0 : 1);
    if (rc) {
        gs_set_error("gs_draw: unsupported flag combination");
        return rc;
    }
    GS_CHECK_LAUNCH();
    return 0;
}
