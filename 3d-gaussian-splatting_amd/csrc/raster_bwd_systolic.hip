// raster_bwd_systolic.hip -- tile rasterizer backward, `sigmoid = True` of the reference API (a rarely used flag): the 64-lane
// systolic pipeline.  The overview of the backward kernels and the gradient identities: raster_bwd.hip.
#include "raster_bwd_common.h"

namespace {

// the systolic kernel (rgb and degree-2 SH colours: what the reference API has)
template <int CDIM>
struct BwdCfg {
    static constexpr int WPB = 4;  // waves per workgroup, one bucket each (they never synchronise)
    // What is constant per pixel (dL/dC, pixel centre) either rides the DPP chain with the pixel's running state or
    // is read by every lane from an LDS table indexed by the pixel it currently holds.  A DPP move costs as much
    // SIMD time as three plain instructions (tools/ubench/pk_rate.hip), a per-lane LDS read costs no VALU slot but
    // LDS bandwidth and 4 KiB per wave.  Measured (cfg2 / cfg4, same run): the table is 9 % faster without SH
    // (issue-bound, 5 waves per SIMD) and 2 % slower with SH (register-limited to 2-3 waves, latency-bound, and
    // the SH basis records already load the LDS pipe).
    static constexpr bool TABLE = CDIM == 3;
    static constexpr int NB = CDIM > 3 ? CDIM / 3 : 1;        // SH basis functions per channel
    static constexpr int SHS = NB;                            // LDS record stride (floats): 9 is conflict-free
};

// The `sigmoid` flag of the reference API's draw / draw_backward -- alpha is squashed,
// alpha = 2 / (1 + e^-a) - 1 with a = p0 G opa, p0 = (pi/2) rsqrt(det + 1e-7) (gaussian.cu:593-594, 918, 930).
// p0 is folded into the lane's opacity; its own cov gradient (gaussian.cu:622-630) only needs sum(dL/da G), which
// is the opacity accumulator, so the loop pays two extra transcendentals and three plain instructions.
// EXACT (reference API, `fast = 0`, gaussian.cu:596-603): the Gaussian's value through a double-precision exp of the
// float argument, as the reference's backward evaluates it; v_exp_f32 otherwise.
template <int CDIM, bool EXACT>
__global__ void __launch_bounds__(64 * BwdCfg<CDIM>::WPB) raster_backward_kernel(RasterSrc S, RasterGeom G, BwdIn I,
                                                                              BwdOut O) {
    static_assert(CDIM == 3 || CDIM == 27, "the reference API has rgb and degree-2 SH colours");
    constexpr int WPB = BwdCfg<CDIM>::WPB, NB = BwdCfg<CDIM>::NB, SHS = BwdCfg<CDIM>::SHS;
    // Feed ring: the 256 pixel states of a bucket enter lane 0 in four segments of 64; while a
    // segment streams through the lanes, the next one is prefetched into registers and then
    // written to the other half of the ring.  ~6 KiB of LDS per wave keeps occupancy
    // register-limited (the dependent DPP chain needs >= 5 waves per SIMD to stay hidden).
    constexpr bool TABLE = BwdCfg<CDIM>::TABLE;
    constexpr int NF = TABLE ? 1 : 2;  // float4 feed records per pixel: (T, rho, -, -) | (T, rho, px, py), (dL/dC, -)
    __shared__ float4 s_feed[WPB][2][NF][64];
    __shared__ float4 s_pix[TABLE ? WPB : 1][TABLE ? 256 : 1];  // TABLE: (dL/dC rgb, pixel centre x) of tile pixel p
    __shared__ float s_py[TABLE ? WPB : 1][16];                 // TABLE: pixel centre y of tile row p >> 4
    // SH only: the 9 basis values of a pixel never change while it travels, so they do not ride the DPP chain
    // (9 moves = 28 ns of SIMD time per step, tools/ubench/pk_rate.hip); they are staged once per bucket and
    // every lane reads the record of the pixel it currently holds (LDS reads, no VALU issue slots).
    __shared__ float s_sh[CDIM > 3 ? WPB : 1][CDIM > 3 ? 256 * SHS : 4] __attribute__((aligned(16)));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n_tiles = (uint32_t)(G.ntx * G.nty);
    const uint32_t kb = blockIdx.x * WPB + wave;
    if (kb >= I.bucket_offsets[n_tiles]) return;  // whole wave exits; no block-level barrier below

    const uint4 info = I.bucket_info[kb];
    const uint32_t tile = info.x, b = info.y / GS_BUCKET;  // bucket -> (tile, local bucket)
    const uint32_t tx = tile % (uint32_t)G.ntx, ty = tile / (uint32_t)G.ntx;
    const uint32_t start = (uint32_t)I.ranges[tile];
    const uint32_t nproc = I.tile_nproc[tile];
    const uint32_t jloc = b * GS_BUCKET + lane;
    const bool gvalid = jloc < nproc;
    const uint32_t j = start + jloc;
    const int nvalid = (int)((nproc - b * GS_BUCKET) < (uint32_t)GS_BUCKET ? (nproc - b * GS_BUCKET) : GS_BUCKET);

    // ---- per-segment staging of the pixel states (pixel p = 64 seg + lane)
    const float4 *ck = I.ckpt + raster_ckpt_slot(start, tile, b) * 256;
    const uint32_t id_x = tx * 16 + (lane & 15);
    const float my_px = raster_pixel_coord(id_x, G.padW, G.focal_x);
    float4 pc;            // prefetched checkpoint (T, C_run)
    float pf0, pf1, pf2;  // final colour
    float pg0, pg1, pg2;  // dL/dC
    auto load_segment = [&](int seg) {
        const int p = seg * 64 + lane;
        const uint32_t id_y = ty * 16 + (p >> 4);
        pc = b == 0 ? make_float4(1.f, 0.f, 0.f, 0.f) : ck[p];  // bucket 0 starts from the empty pixel (not stored)
        float f[3], g[3];
        load_pixel_inputs<false>(I, G, id_x, id_y, f, g);
        pf0 = f[0];
        pf1 = f[1];
        pf2 = f[2];
        pg0 = g[0];
        pg1 = g[1];
        pg2 = g[2];
    };
    auto write_segment = [&](int buf, int seg) {
        const uint32_t id_y = ty * 16 + seg * 4 + (lane >> 4);
        const float py = raster_pixel_coord(id_y, G.padH, G.focal_y);
        // rho = dL/dC . (C_final - C_run): the only way the remaining colour enters dL/dalpha
        // (gaussian.cu:716-722), so one scalar travels instead of three colour channels
        const float rho = pg0 * (pf0 - pc.y) + pg1 * (pf1 - pc.z) + pg2 * (pf2 - pc.w);
        s_feed[wave][buf][0][lane] = make_float4(pc.x, rho, my_px, py);
        if (TABLE) {
            s_pix[wave][seg * 64 + lane] = make_float4(pg0, pg1, pg2, my_px);
            if ((lane & 15) == 0) s_py[wave][seg * 4 + (lane >> 4)] = py;
        } else {
            s_feed[wave][buf][NF - 1][lane] = make_float4(pg0, pg1, pg2, 0.f);
        }
        if (CDIM > 3) {
            float SH[NB];
            raster_pixel_sh<NB>(id_x, id_y, G, SH);
#pragma unroll
            for (int q = 0; q < NB; ++q) s_sh[wave][(seg * 64 + lane) * SHS + q] = SH[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    load_segment(0);
    if (TABLE) {
        // lanes that hold no pixel yet read the records of segment 3 before it is staged: their T is exactly zero,
        // but 0 x (whatever the previous kernel left in LDS, e.g. the tile sort's all-ones padding = NaN) must stay 0
        s_pix[wave][192 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < 4) s_py[wave][12 + lane] = 0.f;
    }
    if (CDIM > 3) {
        // lanes that hold no pixel yet read records of segments that are not staged yet: their weight is exactly
        // zero, but 0 x (whatever the previous kernel left in LDS, e.g. the tile sort's all-ones padding = NaN)
        // must not reach the accumulators
#pragma unroll
        for (int q = 0; q < 4 * SHS; ++q) s_sh[wave][q * 64 + lane] = 0.f;
    }

    // ---- this lane's Gaussian
    GaussianRec g = {0, 0, 0, 0, 0, 0, 0};
    float col0 = 0, col1 = 0, col2 = 0;
    float coef[CDIM > 3 ? CDIM : 1];
    uint32_t gid = 0;
    if (gvalid) {
        gid = raster_load<false>(S, j, g);
        if (CDIM == 3) {
            raster_load_rgb<false>(S, j, gid, col0, col1, col2);
        } else {
            const float *src = raster_sh_ptr<false, CDIM>(S, j, gid);
#pragma unroll
            for (int q = 0; q < CDIM; ++q) coef[q] = src[q];
        }
    } else if (CDIM > 3) {
#pragma unroll
        for (int q = 0; q < CDIM; ++q) coef[q] = 0.f;
    }
    float cA = 0, cB = 0, cC = 0;
    if (gvalid) raster_conic(g, cA, cB, cC);
    float opa = gvalid ? g.opa : 0.f;  // opacity 0 => alpha 0 => state passes through unchanged
    const float p0 = 1.5707963268f * rsqrtf(raster_det(g.a, g.b, g.c, g.d) + 1e-7f);
    opa *= p0;  // the same folding as the forward kernel (raster_fwd_body.h)
    write_segment(0, 0);

    // gradient accumulators
    float Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0, Sq = 0, Sopa = 0, Sc0 = 0, Sc1 = 0, Sc2 = 0;
    float Ssh[CDIM > 3 ? CDIM : 1];
    if (CDIM > 3) {
#pragma unroll
        for (int q = 0; q < CDIM; ++q) Ssh[q] = 0.f;
    }
    // outgoing state of the previous step (T = 0 means "no pixel here")
    float oT = 0, orho = 0, og0 = 0, og1 = 0, og2 = 0, opx = 0, opy = 0;

    for (int seg = 0; seg < 5; ++seg) {
        const int buf = seg & 1;
        if (seg + 1 < 4) load_segment(seg + 1);  // in flight while this segment streams
        const bool feeding = seg < 4;
        // drain: the last pixel leaves lane nvalid-1 after nvalid-1 more steps; rounded up to an even count (the
        // extra step moves an empty slot) so that the loop unrolls by two without a remainder loop, which the
        // convergent DPP moves forbid
        const int nsteps = feeding ? 64 : (nvalid & ~1);
        auto step = [&](const int t) {
            // feed for lane 0 (broadcast LDS reads; while draining feed T = 0)
            const float4 f0 = s_feed[wave][buf][0][t];
            const float fT = feeding ? f0.x : 0.f;
            // state entering this lane: lane l-1's output of the previous step; lane 0 takes the feed
            const float T = gs_wave_shr1(fT, oT);
            float rho = gs_wave_shr1(f0.y, orho);
            // the pixel in this lane entered lane 0 `lane` steps ago: p = 64 seg + t - lane (lanes that hold no
            // pixel yet / any more read a valid but irrelevant record: their T is 0)
            const int p = (seg * 64 + t - lane) & 255;
            float px, py, g0, g1, g2;
            if (TABLE) {
                const float4 pr = s_pix[wave][p];
                g0 = pr.x, g1 = pr.y, g2 = pr.z, px = pr.w, py = s_py[wave][p >> 4];
            } else {
                const float4 f1 = s_feed[wave][buf][NF - 1][t];
                px = gs_wave_shr1(f0.z, opx), py = gs_wave_shr1(f0.w, opy);
                g0 = gs_wave_shr1(f1.x, og0), g1 = gs_wave_shr1(f1.y, og1), g2 = gs_wave_shr1(f1.z, og2);
            }
            float sh[NB];
            if (CDIM > 3) {
                const float *rec = &s_sh[wave][p * SHS];
#pragma unroll
                for (int q = 0; q < NB; ++q) sh[q] = rec[q];
            }

            const float dx = px - g.x, dy = py - g.y;
            const float q = fmaf(cC * dy, dy, dx * fmaf(-cB, dy, cA * dx));  // same evaluation order as the forward
            const float Gv = EXACT ? (float)exp(-(double)(q * GS_LN2)) : gs_exp2(-q);
            const bool live = T > GS_T_STOP;
            const float araw = live ? Gv * opa : 0.f;  // before squashing
            const float alpha = gs_squash_alpha(araw);
            const float w = alpha * T;
            if (CDIM > 3) {
                float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    v0 = fmaf(sh[k], coef[k], v0);
                    v1 = fmaf(sh[k], coef[NB + k], v1);
                    v2 = fmaf(sh[k], coef[2 * NB + k], v2);
                }
                col0 = gs_rcp(1.0f + __expf(-v0));
                col1 = gs_rcp(1.0f + __expf(-v1));
                col2 = gs_rcp(1.0f + __expf(-v2));
            }
            // dL/dC . colour of this Gaussian, and rho AFTER it (the reference's cur_out - color, :719)
            const float gc = fmaf(g2, col2, fmaf(g1, col1, g0 * col0));
            rho = fmaf(-w, gc, rho);
            const float one_m = 1.0f - alpha;
            float d_alpha = fmaf(T, gc, -(rho * gs_rcp(one_m + 1e-7f)));
            d_alpha = live ? d_alpha : 0.f;
            d_alpha *= (alpha + 1.0f) - 0.5f * (alpha + 1.0f) * (alpha + 1.0f);  // d squash / da, :727
            if (CDIM > 3) {
                const float D0 = g0 * w * (col0 * (1.0f - col0)), D1 = g1 * w * (col1 * (1.0f - col1)),
                            D2 = g2 * w * (col2 * (1.0f - col2));
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    Ssh[k] = fmaf(D0, sh[k], Ssh[k]);
                    Ssh[NB + k] = fmaf(D1, sh[k], Ssh[NB + k]);
                    Ssh[2 * NB + k] = fmaf(D2, sh[k], Ssh[2 * NB + k]);
                }
            } else {
                Sc0 = fmaf(g0, w, Sc0);
                Sc1 = fmaf(g1, w, Sc1);
                Sc2 = fmaf(g2, w, Sc2);
            }
            Sopa = fmaf(d_alpha, Gv, Sopa);
            const float s = d_alpha * araw;
            const float sdx = s * dx, sdy = s * dy;
            Sx += sdx;
            Sy += sdy;
            Sxx = fmaf(sdx, dx, Sxx);
            Sxy = fmaf(sdx, dy, Sxy);
            Syy = fmaf(sdy, dy, Syy);
            Sq = fmaf(s, q, Sq);
            // outgoing state
            oT = fmaf(-alpha, T, T);  // identical to the forward's update
            orho = rho;
            og0 = g0;
            og1 = g1;
            og2 = g2;
            opx = px;
            opy = py;
        };
        for (int t = 0; t < nsteps; t += 2) {  // nsteps is even: two steps per iteration, no remainder loop
            step(t);
            step(t + 1);
        }
        if (seg + 1 < 4) write_segment(buf ^ 1, seg + 1);
    }

    if (!gvalid) return;
    const float det = raster_det(g.a, g.b, g.c, g.d);
    const float iPn = 1.0f / (2.0f * det + 1e-14f);
    const float Su = Sq * GS_LN2;  // u = -ln G = q ln 2
    const float gx = GS_LN2 * (2.0f * cA * Sx - cB * Sy);
    const float gy = GS_LN2 * (2.0f * cC * Sy - cB * Sx);
    float ga = iPn * (-Syy + 2.0f * g.d * Su);
    float gb = iPn * (Sxy - 2.0f * g.c * Su);
    float gc = iPn * (Sxy - 2.0f * g.b * Su);
    float gd = iPn * (-Sxx + 2.0f * g.a * Su);
    // dp0/d{a,b,c,d} = k0 (-d, c, b, -a), k0 = p0^3 / (2 (pi/2)^2) (gaussian.cu:622-626), times
    // sum_pixels dL/da G opa_raw (:740-744); Sopa so far is sum dL/da G
    const float k0 = 0.5f * (p0 * p0 * p0) / (1.5707963268f * 1.5707963268f) * Sopa * g.opa;
    ga -= k0 * g.d;
    gb += k0 * g.c;
    gc += k0 * g.b;
    gd -= k0 * g.a;
    Sopa *= p0;  // dL/dopa = sum dL/da (p0 G)
    O.grad_pos[(size_t)j * 3 + 0] = gx;
    O.grad_pos[(size_t)j * 3 + 1] = gy;
    O.grad_opa[j] = Sopa;
    reinterpret_cast<float4 *>(O.grad_cov)[j] = make_float4(ga, gb, gc, gd);
    if (CDIM == 3) {
        O.grad_rgb[(size_t)j * 3 + 0] = Sc0;
        O.grad_rgb[(size_t)j * 3 + 1] = Sc1;
        O.grad_rgb[(size_t)j * 3 + 2] = Sc2;
    } else {
#pragma unroll
        for (int k = 0; k < CDIM; ++k) O.grad_rgb[(size_t)j * CDIM + k] = Ssh[k];
    }
}

// four buckets per workgroup
template <int CDIM>
void launch_systolic(int exact, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O, int64_t max_buckets,
                     hipStream_t stream) {
    constexpr int WPB = BwdCfg<CDIM>::WPB;
    const int grid = (int)gs_div_up(max_buckets > 0 ? max_buckets : 1, WPB);
    if (exact)
        hipLaunchKernelGGL((raster_backward_kernel<CDIM, true>), dim3(grid), dim3(64 * WPB), 0, stream, S, G, I, O);
    else
        hipLaunchKernelGGL((raster_backward_kernel<CDIM, false>), dim3(grid), dim3(64 * WPB), 0, stream, S, G, I, O);
}

}  // namespace

void gs_launch_bwd_systolic(int color_dim, int exact, const RasterSrc &S, const RasterGeom &G, const BwdIn &I, const BwdOut &O,
                            int64_t max_buckets, hipStream_t stream) {
    if (color_dim == 27)
        launch_systolic<27>(exact, S, G, I, O, max_buckets, stream);
    else
        launch_systolic<3>(exact, S, G, I, O, max_buckets, stream);
}
