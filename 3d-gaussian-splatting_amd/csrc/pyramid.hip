// pyramid.hip -- one level down of an image pyramid for coarse-to-fine camera tracking (gs_pyramid_down; include/gs_abi.h):
// the colour target box-filtered 2 x 2 and a measurement-aware range target, one launch.
//
// Coarse pixel (i, j) covers the fine pixels (2i..2i+1, 2j..2j+1), named 00, 01, 10, 11 in row-major order.  Per coarse
// pixel, in fp32 with one rounding per operation (this file is compiled -ffp-contract=off):
//   colour, per channel:  ((a00 + a01) + a10) + a11, times 0.25f (exact short of underflow).  No rule for NaN: it propagates.
//   range:  a fine pixel is measured iff map_measured (map_terms.h: > 0 and finite -- the rule of gs_loss_depth and
//           gs_loss_track); n = how many of the four are, lo / hi = their minimum / maximum;
//           the coarse pixel is measured iff n >= min_valid and (edge_rel < 0 or hi <= fl(fl(1 + edge_rel) lo));
//           its value is s / (float)n, s = ((v00 + v01) + v10) + v11 with v = the range where measured and +0.0f where not;
//           an unmeasured coarse pixel is written as exactly 0.0f.
// The edge test drops a footprint that straddles a depth discontinuity: the mean of a near and a far surface is a range no
// surface has.  The coarse pixel's ray passes through the corner its four fine pixels share; the mean of four ranges along
// four slightly different rays is a second-order approximation of the range along that ray -- targets for tracking, not for
// seeding or mapping.
//
// Geometry (track_loss_kernel's: one streaming pass, 16-byte accesses).  An ITEM is four consecutive coarse pixels of one
// coarse row -- fewer at the end of a row whose width is no multiple of four; a coarse row has Q = ceil((W / 2) / 4) items and
// the image (H / 2) Q, numbered row by row.  A lane takes one item: two fine rows of eight pixels.  A workgroup is 256 lanes
// = 256 consecutive items (1,024 coarse pixels when W / 2 is a multiple of four); its share ends inside a row whenever Q does
// not divide 256, and the last workgroup is partial whenever 256 does not divide (H / 2) Q.  The grid is
// ceil((H / 2) Q / 256) workgroups, one item per lane: there is NO grid cap and no loop over items (an image of 2^31 items
// or more is refused).
//   W % 8 == 0: every fine row and every coarse row starts on a 16-byte boundary and W / 2 is a multiple of four -- a lane
//               issues 12 + 4 16-byte loads (colour, range) and 3 + 1 16-byte stores, no tails.
//   otherwise : the same items pixel by pixel with 4-byte accesses (a row's last item holds one to three pixels).
// 16 bytes in and 4 out per fine pixel against a dozen operations: bound by memory traffic.  No atomics, no LDS, no scratch;
// every store is a vector store or plain C++.  Two instantiations, <RANGE>.
#include <cmath>

#include "gs_common.h"
#include "map_terms.h"  // map_measured

namespace {

constexpr int PD_BLOCK = 256;

__device__ __forceinline__ float pyramid_colour(float a00, float a01, float a10, float a11) {
    return (((a00 + a01) + a10) + a11) * 0.25f;
}

__device__ __forceinline__ float pyramid_range(float v00, float v01, float v10, float v11, int min_valid, float edge_rel,
                                               float one_plus) {
    const bool m00 = map_measured(v00), m01 = map_measured(v01), m10 = map_measured(v10), m11 = map_measured(v11);
    const int n = (int)m00 + (int)m01 + (int)m10 + (int)m11;
    v00 = m00 ? v00 : 0.f;
    v01 = m01 ? v01 : 0.f;
    v10 = m10 ? v10 : 0.f;
    v11 = m11 ? v11 : 0.f;
    float lo = INFINITY, hi = 0.f;  // (over the measured ones: all positive and finite)
    if (m00) lo = fminf(lo, v00), hi = fmaxf(hi, v00);
    if (m01) lo = fminf(lo, v01), hi = fmaxf(hi, v01);
    if (m10) lo = fminf(lo, v10), hi = fmaxf(hi, v10);
    if (m11) lo = fminf(lo, v11), hi = fmaxf(hi, v11);
    const float s = ((v00 + v01) + v10) + v11;
    const bool ok = n >= min_valid && (edge_rel < 0.f || hi <= one_plus * lo);  // (min_valid >= 1: n == 0 never passes)
    return ok ? s / (float)n : 0.f;
}

template <bool RANGE>
__global__ void __launch_bounds__(PD_BLOCK)
    pyramid_down_kernel(const float *__restrict__ image, const float *__restrict__ range, int32_t Wc, uint32_t Q, uint32_t items,
                        int vec, int min_valid, float edge_rel, float one_plus, float *__restrict__ image_out,
                        float *__restrict__ range_out) {
    const uint32_t item = blockIdx.x * PD_BLOCK + threadIdx.x;  // (the host keeps items below 2^31)
    if (item >= items) return;
    const uint32_t i = item / Q, q = item - i * Q;  // coarse row, item of the row
    const int64_t W = 2 * (int64_t)Wc, j0 = 4 * (int64_t)q;
    const int64_t fine = (2 * (int64_t)i) * W + 2 * j0, coarse = (int64_t)i * Wc + j0;  // first fine / coarse pixel
    if (vec) {
        float a[24], b[24];  // the eight pixels of the upper and of the lower fine row, in memory order
        const float4 *pa = reinterpret_cast<const float4 *>(image + fine * 3);
        const float4 *pb = reinterpret_cast<const float4 *>(image + (fine + W) * 3);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float4 u = pa[k], v = pb[k];
            a[4 * k] = u.x, a[4 * k + 1] = u.y, a[4 * k + 2] = u.z, a[4 * k + 3] = u.w;
            b[4 * k] = v.x, b[4 * k + 1] = v.y, b[4 * k + 2] = v.z, b[4 * k + 3] = v.w;
        }
        float c[12];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                c[p * 3 + ch] = pyramid_colour(a[6 * p + ch], a[6 * p + 3 + ch], b[6 * p + ch], b[6 * p + 3 + ch]);
        float4 *po = reinterpret_cast<float4 *>(image_out + coarse * 3);
        po[0] = make_float4(c[0], c[1], c[2], c[3]);
        po[1] = make_float4(c[4], c[5], c[6], c[7]);
        po[2] = make_float4(c[8], c[9], c[10], c[11]);
        if (RANGE) {
            const float4 *ra = reinterpret_cast<const float4 *>(range + fine);
            const float4 *rb = reinterpret_cast<const float4 *>(range + fine + W);
            const float4 u0 = ra[0], u1 = ra[1], v0 = rb[0], v1 = rb[1];
            float4 z;
            z.x = pyramid_range(u0.x, u0.y, v0.x, v0.y, min_valid, edge_rel, one_plus);
            z.y = pyramid_range(u0.z, u0.w, v0.z, v0.w, min_valid, edge_rel, one_plus);
            z.z = pyramid_range(u1.x, u1.y, v1.x, v1.y, min_valid, edge_rel, one_plus);
            z.w = pyramid_range(u1.z, u1.w, v1.z, v1.w, min_valid, edge_rel, one_plus);
            *reinterpret_cast<float4 *>(range_out + coarse) = z;
        }
    } else {
        const int np = (int)(Wc - j0 < 4 ? Wc - j0 : 4);  // a row's last item may hold one to three pixels
        for (int p = 0; p < np; ++p) {
            const float *pa = image + (fine + 2 * p) * 3, *pb = pa + W * 3;
            float *po = image_out + (coarse + p) * 3;
            po[0] = pyramid_colour(pa[0], pa[3], pb[0], pb[3]);
            po[1] = pyramid_colour(pa[1], pa[4], pb[1], pb[4]);
            po[2] = pyramid_colour(pa[2], pa[5], pb[2], pb[5]);
            if (RANGE) {
                const float *ra = range + fine + 2 * p, *rb = ra + W;
                range_out[coarse + p] = pyramid_range(ra[0], ra[1], rb[0], rb[1], min_valid, edge_rel, one_plus);
            }
        }
    }
}

inline bool pyramid_overlap(const void *p, size_t np, const void *q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" int gs_pyramid_down(const float *image, const float *range, int32_t H, int32_t W, const gs_pyramid_opts *opts,
                               float *image_out, float *range_out, gs_stream_t stream) {
    GS_CHECK_ARG(image && image_out && opts, "null pointer: image, image_out and opts must be given");
    GS_CHECK_ARG((range == nullptr) == (range_out == nullptr),
                 "range and range_out must both be NULL (RGB only) or both be given");
    GS_CHECK_ARG(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "H and W must be positive and even");
    {
        const void *al[] = {image, range, image_out, range_out};
        const char *what[] = {"image must be 16-byte aligned", "range must be 16-byte aligned",
                              "image_out must be 16-byte aligned", "range_out must be 16-byte aligned"};
        for (int k = 0; k < 4; ++k) GS_CHECK_ARG(((uintptr_t)al[k] & 15) == 0, what[k]);
    }
    GS_CHECK_ARG(opts->min_valid >= 1 && opts->min_valid <= 4, "min_valid must be 1..4");
    GS_CHECK_ARG(!std::isnan(opts->edge_rel), "edge_rel must not be NaN (negative: the edge test is off)");
    const int64_t Hc = H / 2, Wc = W / 2, Q = (Wc + 3) / 4, items = Hc * Q;
    GS_CHECK_ARG(items <= 0x7fffffff, "image size beyond 2^31 groups of four coarse pixels");
    {
        const size_t n_in = (size_t)H * (size_t)W * sizeof(float), n_out = (size_t)Hc * (size_t)Wc * sizeof(float);
        bool ov = pyramid_overlap(image_out, 3 * n_out, image, 3 * n_in);
        if (range)
            ov = ov || pyramid_overlap(image_out, 3 * n_out, range, n_in) || pyramid_overlap(range_out, n_out, image, 3 * n_in) ||
                 pyramid_overlap(range_out, n_out, range, n_in);
        GS_CHECK_ARG(!ov, "an output overlaps an input (no level is made in place)");
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)gs_div_up(items, PD_BLOCK);
    const int vec = W % 8 == 0;
    const float one_plus = 1.f + opts->edge_rel;  // fl(1 + edge_rel): one rounding, then one more in the product with lo
    if (range)
        hipLaunchKernelGGL(pyramid_down_kernel<true>, dim3(blocks), dim3(PD_BLOCK), 0, s, image, range, (int32_t)Wc, (uint32_t)Q,
                           (uint32_t)items, vec, opts->min_valid, opts->edge_rel, one_plus, image_out, range_out);
    else
        hipLaunchKernelGGL(pyramid_down_kernel<false>, dim3(blocks), dim3(PD_BLOCK), 0, s, image, range, (int32_t)Wc,
                           (uint32_t)Q, (uint32_t)items, vec, opts->min_valid, opts->edge_rel, one_plus, image_out, range_out);
    GS_CHECK_LAUNCH();
    return 0;
}
