// raster_fwd_common.h -- what more than one of the forward compositing files needs: the LDS layout of a chunk, the packed-float
// helpers, the tuning macros, the grid plan of the launches and the segment stage's entry.
//   raster_fwd_body.h       the compositing kernel (raster_forward_body and its two __global__ wrappers, launch_fwd)
//   raster_fwd.hip          the frame path: gs_stage_raster_forward
//   raster_fwd_ref.hip      the reference API: gs_draw, gs_raster_forward_ref
//   raster_fwd_segment.hip  dense frames: segmented compositing of long tile lists, gs_stage_raster_segments
// Everything but that entry sits in an anonymous namespace, as it did in the one file: the kernels' symbols are unchanged,
// and each translation unit launches its own.
#pragma once
#include <stdlib.h>

#include "raster_common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int FWD_THREADS = 64;  // ONE wave64 per 16x16 tile, 4 pixels per lane
constexpr int NPP = 2;           // pixel pairs per lane
#ifndef GS_FWD_WAVES_PER_SIMD
#define GS_FWD_WAVES_PER_SIMD 8
#endif

template <int CDIM>
struct FwdSmem {  // SH: CDIM = 27 (degree 2) or 48 (degree 3) raw coefficients per Gaussian, channel-major
    static constexpr int CH = 64;
    static constexpr int NB = CDIM / 3;
    static constexpr int SHS = CDIM == 27 ? 28 : CDIM + 4;  // record stride: 16-byte rows, 4-way conflicts on the fill
    enum { X, Y, A, B, C, NLOP, DH, DL, NFIELD };  // DH, DL: exact-exp flavour only (see FwdSmem<3>)
    // ONE buffer: the single wave stages chunk k + 1 after it has composited chunk k (LDS operations of a wave execute in
    // order), and the coefficients are loaded in the iteration that consumes them anyway; a second buffer only halved
    // the waves per SIMD (17 / 30 KiB per wave: 2 / 1 waves per SIMD for degree 2 / 3)
    static constexpr int NBUF = 1;
    float f[NBUF][NFIELD][CH] __attribute__((aligned(16)));
    float sh[NBUF][CH][SHS] __attribute__((aligned(16)));
};
template <>
struct FwdSmem<3> {
    // structure of arrays: four consecutive Gaussians of one field are one ds_read_b128
    static constexpr int CH = 64;
    // NLOP = -log2(opacity) (frame path) or the opacity (reference API).  Exact-exp flavour of the reference API
    // (`fast = 0`, gaussian.cu:922-923): A, B, C hold the raw covariance entries a, b + c, d and DH + DL the double
    // 2 det + 1e-14 as two floats (48 of its 53 bits)
    enum { X, Y, A, B, C, NLOP, R, G, BL, DH, DL, NFIELD };
    static constexpr int NBUF = 2;
    float f[NBUF][NFIELD][CH] __attribute__((aligned(16)));
};

__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// a * b with DX9 zero rules: 0 x anything (NaN, infinity) = 0 (v_mul_legacy_f32).  Declared as the LLVM intrinsic, NOT
// as inline assembly: the operand is the result of a transcendental (v_exp_f32), which on gfx940/950 needs a wait state
// before a VALU instruction may read it -- the compiler inserts it for instructions it knows, not for opaque asm text
// (first version: stale alphas in a few pixels per frame).
extern "C" __device__ float gs_fmul_legacy(float, float) __asm("llvm.amdgcn.fmul.legacy");
__device__ __forceinline__ float mul_legacy(float a, float b) { return gs_fmul_legacy(a, b); }

// Exact per-pixel liveness in ONE packed instruction: m = clamp((t - 0.0001f) * 2^100) is 1.0 when
// t > 0.0001f and 0.0 otherwise (the fma is exact up to its final rounding, and the smallest positive
// t - 0.0001f is one ulp of 1e-4, which 2^100 lifts far above 1).  Replaces v_cmp + v_cndmask per pixel.
#define GS_LIVE_SCALE 1.2676506002282294e30f /* 2^100 */
__device__ __forceinline__ f2 live_mask(f2 t, f2 scale, f2 bias) {
    f2 m;
    asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(m) : "v"(t), "v"(scale), "v"(bias));
    return m;
}

#ifndef GS_FWD_RGB_WPE
#define GS_FWD_RGB_WPE 4  // rgb colours: four waves per SIMD asked for.  Left to itself the allocator gave the training variant
                         // (checkpoint stores) 130 VGPRs = three waves; with the hint it fits 128 without scratch: training
                         // forward at 2.4 M Gaussians 136 -> 129 us, inference 126 VGPRs, +-1 % (same-box A/B, round 3)
#endif
#ifndef GS_FWD_COMPACT_MIN
#define GS_FWD_COMPACT_MIN 16  // rgb inference frames: the Gaussians a list must have left for a tile to compact (the compact
                               // phase, raster_fwd_body.h).  Measured with 8 / 16 / 32: 4,807 / 4,758 - 4,800 / 4,789 FPS on the
                               // headline scene, all within one build's own spread (profiles/raster_compact_ab.txt): 16 stays
#endif
#ifndef GS_FWD_SH27_WPE
#define GS_FWD_SH27_WPE 3  // waves per SIMD the register allocation of the SH kernels aims at (A/B switches; degree 2 at
                           // 3: 168 VGPRs and 22 spilled outside the loop, 0.535 -> 0.510 ms at 2.4 M Gaussians)
#endif
#ifndef GS_FWD_SH48_WPE
#define GS_FWD_SH48_WPE 2
#endif

// Staging an rgb Gaussian: a NaN colour must reach the LIVE pixels only (the reference never evaluates the Gaussian for a
// finished one); 0 x NaN in the colour FMAs would poison every pixel, so the NaN is moved into the staged opacity `nlop`, where
// the DX9 multiply (or the select that stands for it) confines it to live pixels, and the colour becomes 0 (0 x NaN = NaN there)
__device__ __forceinline__ void fwd_confine_nan_colour(float &r0, float &r1, float &r2, float &nlop) {
    if (r0 != r0 || r1 != r1 || r2 != r2) {
        nlop = __builtin_nanf("");
        r0 = r1 = r2 = 0.f;
    }
}

// One finished pixel (o0, o1, o2) at (id_x, id_y) of the padded frame: the padded image, and the clamped, centre-cropped one.
__device__ __forceinline__ void fwd_store_pixel(const RasterGeom &G, float *out_padded, float *out_image, uint32_t id_x,
                                                uint32_t id_y, float o0, float o1, float o2) {
    if (out_padded) {
        float *o = out_padded + ((size_t)id_y * G.padW + id_x) * 3;
        o[0] = o0;
        o[1] = o1;
        o[2] = o2;
    }
    if (out_image) {  // clamp + centred crop (splatter.py:652-653, 267-272)
        const int ox = (int)id_x - G.crop_left, oy = (int)id_y - G.crop_top;
        if (ox >= 0 && ox < G.width && oy >= 0 && oy < G.height) {
            float *o = out_image + ((size_t)oy * G.width + ox) * 3;
            // torch.clamp semantics: NaN stays NaN (fminf / fmaxf would turn it into 0)
            o[0] = o0 > 1.f ? 1.f : (o0 < 0.f ? 0.f : o0);
            o[1] = o1 > 1.f ? 1.f : (o1 < 0.f ? 0.f : o1);
            o[2] = o2 > 1.f ? 1.f : (o2 < 0.f ? 0.f : o2);
        }
    }
}

// Outputs of the depth / alpha maps (GS_FRAME_AUX): raster_aux_forward_kernel passes them, the plain kernel an empty set.
struct AuxFwdOut {
    float2 *padded;  // [padH, padW] (D, A) raw sums
    float *depth;    // [H, W] cropped, may be NULL
    float *alpha;    // [H, W] cropped, may be NULL
    float2 *ckpt;    // training: [max_buckets][256] (D, A) at bucket starts (the slots of the colour checkpoints)
};

// Waves in the grid: every wave gets the same number of tiles (+-1) and there are at most GS_FWD_WAVES_PER_SIMD
// (default 8) waves per SIMD -- at 1080p that is one tile per wave, dispatched by the hardware in index order as slots
// free up (with tile_order: longest-first list scheduling); fewer, longer-lived waves were slower (122-154 us against
// 85 us at cfg2).  The slot count is cached from the first device seen (all GPUs of a node are the same part).
struct FwdPlan {
    int slots;  // wave slots of the device at GS_FWD_WAVES_PER_SIMD
    int order;  // use tile_order (default 1; GS_FWD_ORDER=0 in the environment switches it off: A/B measurements)
};
static const FwdPlan &fwd_plan() {
    static const FwdPlan plan = [] {
        FwdPlan p;
        hipDeviceProp_t prop;
        int dev = 0, wps = GS_FWD_WAVES_PER_SIMD, cus = 256;
        if (const char *e = getenv("GS_FWD_WAVES_PER_SIMD")) wps = atoi(e) > 0 ? atoi(e) : wps;  // tuning knob
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        p.slots = cus * 4 * wps;
        const char *o = getenv("GS_FWD_ORDER");
        p.order = o ? atoi(o) != 0 : 1;
        return p;
    }();
    return plan;
}
static uint32_t fwd_grid(uint32_t n_tiles) {
    const FwdPlan &p = fwd_plan();
    const uint32_t rounds = (n_tiles + p.slots - 1) / p.slots;
    return rounds ? (n_tiles + rounds - 1) / rounds : 1;
}
// The grid of a compositing launch over n_tiles tiles.  The gated second pass of a culled frame almost never runs: a small
// persistent grid (every wave walks several tiles) returns in ~2 us where n_tiles workgroups take ~8 us to be dispatched and
// retired.
static uint32_t fwd_launch_grid(uint32_t n_tiles, const unsigned long long *gate) {
    return gate ? (n_tiles < 1024u ? n_tiles : 1024u) : fwd_grid(n_tiles);
}
// The dispatch order a launch passes to its kernel: the caller's, unless GS_FWD_ORDER=0 switched it off.
static const uint32_t *fwd_tile_order(const uint32_t *tile_order) { return fwd_plan().order ? tile_order : nullptr; }

}  // namespace

// Dense frames (raster_fwd_segment.hip): the rest of every list that gs_stage_raster_forward's launch flagged in ws.cont_flag
// -- scan, the two segment passes, combine --, issued on `stream` behind that launch.
int gs_stage_raster_segments(const gs_frame *f, const gs_frame_ws &ws, const RasterSrc &S, const RasterGeom &G,
                             hipStream_t stream);
