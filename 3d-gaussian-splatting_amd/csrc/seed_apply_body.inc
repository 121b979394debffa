// seed_apply_body.inc -- the body of seed_apply_kernel and of seed_apply_pp_kernel (seed.hip), expanded in place in both.
// Expects in scope: the kernels' parameters, CD, `constexpr bool PP` and -- PP -- pp_dx, pp_dy.  (Included rather than called:
// an inlined device function leaves the kernel of a centred camera with other register assignments than before the variant
// existed; expanded in place, it compiles to the same code.)
    __shared__ float s_dc[CD == 3 ? 1 : SEED_WAVES][CD == 3 ? 1 : 64][3];
    const int64_t need = counts[0];
    if (offset + need > capacity) return;  // (the whole grid alike; the host reads the same count)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long *m = masks + (size_t)blockIdx.x * SEED_WAVES;
    int64_t wave_base = block_offsets[blockIdx.x].x;
#pragma unroll
    for (int w = 0; w < SEED_WAVES - 1; ++w) wave_base += w < wave ? __popcll(m[w]) : 0;
    const unsigned long long mine = m[wave];
    const int rank_in_wave = __popcll(mine & ((1ull << lane) - 1ull));
    const int64_t rank = wave_base + rank_in_wave;
    // (rank < need always holds for the workspace and counts of ONE classify call; the test keeps a mismatched pair in bounds)
    const bool sel = ((mine >> lane) & 1ull) != 0 && rank < need;
    if (sel) {
        const int64_t j = (int64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
        int32_t x, y;
        const int64_t p = seed_pixel(G, j, x, y);
        const float z = range[p];
        float un = (float)(x + P.x0) + 0.5f, vn = (float)(y + P.y0) + 0.5f;
        if (PP) {
            un = un - pp_dx;
            vn = vn - pp_dy;
        }
        const float u = un / P.fx, v = vn / P.fy;
        const float zc = z / sqrtf(u * u + v * v + 1.0f);
        const float q0 = u * zc - P.tran[0], q1 = v * zc - P.tran[1], q2 = zc - P.tran[2];
        const int64_t dst = offset + rank;
#pragma unroll
        for (int k = 0; k < 3; ++k) O.pos[dst * 3 + k] = P.rot[k] * q0 + P.rot[3 + k] * q1 + P.rot[6 + k] * q2;
        const float sigma = P.k_sigma * zc / P.f_mean;
        const float s = P.scale_act == 0 ? fmaxf(sigma - 1e-4f, 0.f) : logf(sigma);
#pragma unroll
        for (int k = 0; k < 3; ++k) O.scale[dst * 3 + k] = s;
        *reinterpret_cast<float4 *>(O.quat + dst * 4) = make_float4(1.f, 0.f, 0.f, 0.f);
        O.opa[dst] = P.opa_logit;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = fminf(fmaxf(image[p * 3 + k], SEED_COLOR_MIN), 1.0f - SEED_COLOR_MIN);
            const float lg = logf(c / (1.0f - c));
            if (CD == 3)
                O.rgb[dst * 3 + k] = lg;
            else
                s_dc[wave][rank_in_wave][k] = lg / SEED_SH_C0;
        }
    }
    if (CD != 3) {
        constexpr int NB = CD / 3;
        __syncthreads();
        // the wave's selected pixels are the consecutive rows [wave_base, wave_base + cnt): cnt * CD consecutive floats
        const int64_t cnt = min((int64_t)__popcll(mine), need - wave_base);
        float *row0 = O.rgb + (offset + wave_base) * CD;
        for (int64_t e = lane; e < cnt * CD; e += 64) {
            const int r = (int)(e / CD), k = (int)(e - (int64_t)r * CD);
            const int c = k / NB;
            row0[e] = k == c * NB ? s_dc[wave][r][c] : 0.f;
        }
    }
