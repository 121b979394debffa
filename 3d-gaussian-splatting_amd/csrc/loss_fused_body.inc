// loss_fused_body.inc -- the body of the fused streaming loss kernel of loss.hip, included once per kernel: with
// GS_LOSS_WEIGHTED 0 it is loss_fused_kernel's text, token for token; with 1 the per-pixel weight map `m` [H, W] enters at
// three places -- the SSIM sum, the three adjoints stage P writes, the L1 / sign term at emit.  (An include and not a device
// function, as frame_project_backward_body.inc: a function changed the plain kernels' registers there.)
    constexpr int LW = FT + 2 * FHALO;
    // every LDS row is double-buffered by the parity of the step, so that ONE barrier per step suffices: step n reads
    // the image row n and the adjoint row n - 1 and writes the image row n + 1 and the adjoint row n into the other halves
    // (round 5: x and y interleaved, and the first two adjoints: one 8-byte read per tap feeds a packed fp32 instruction)
    typedef float f2 __attribute__((ext_vector_type(2)));
    __shared__ f2 s_xy[2][LW];
    __shared__ f2 s_d01[2][LW];
    __shared__ float s_d2[2][LW];
    __shared__ float s_red[FT / 64];
    const int t = threadIdx.x;
    const int F = 3 * L.W;
    const int c0 = blockIdx.x * FCW, r0 = blockIdx.y * SH;
    const int cv = c0 - FHALO + t;                     // this thread's column (may lie outside the image)
    const int pxv = cv >= 0 ? cv / 3 : -1;
    const bool col_in = cv < F && pxv >= R && pxv < L.W - R;          // the SSIM window fits horizontally
    const bool out_col = t >= FHALO && t < FT - FHALO && cv < F;      // this thread stores a gradient column
    // columns of the two LDS slots this thread fills (clamped: values outside the image only reach masked results)
    const int ca = min(max(c0 - 2 * FHALO + t, 0), F - 1), cb = min(max(c0 - 2 * FHALO + FT + t, 0), F - 1);
    const int co = min(max(cv, 0), F - 1);
    auto row_ptr = [&](const float *base, int i) { return base + (size_t)min(max(i, 0), L.H - 1) * F; };
#if GS_LOSS_WEIGHTED
    // A weight multiplies what its own pixel contributes -- S and the adjoints BEFORE the second filter, |x - y| and its sign --
    // so no tap ever needs one: a thread reads the weight of its own column only, whose pixel index is formed once, here.
    const int pm = co / 3;
    auto weight_at = [&](int i) { return m[(size_t)min(max(i, 0), L.H - 1) * L.W + pm]; };
#endif
    float xa, ya, xb = 0.f, yb = 0.f;
    auto fetch = [&](int i) {
        const float *px = row_ptr(x, i), *py = row_ptr(y, i);
        xa = px[ca];
        ya = py[ca];
        if (t < 2 * FHALO) {
            xb = px[cb];
            yb = py[cb];
        }
    };
    auto stage = [&](int buf) {
        s_xy[buf][t] = f2{xa, ya};
        if (t < 2 * FHALO) s_xy[buf][FT + t] = f2{xb, yb};
    };
    if (t < FHALO) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // never written again, read by idle columns
            s_d01[q][t] = s_d01[q][FT + FHALO + t] = f2{0.f, 0.f};
            s_d2[q][t] = s_d2[q][FT + FHALO + t] = 0.f;
        }
    }
    // the rings, in pairs for the packed instructions: (mu, nu), (Exx, Eyy), Exy; (D_mu, D_xx), D_xy
    f2 a1p[K][2], a2p[K];
    float a1s[K], a2s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        a1p[k][0] = a1p[k][1] = a2p[k] = f2{0.f, 0.f};
        a1s[k] = a2s[k] = 0.f;
    }
    auto pfma = [](f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); };
    float ssim_sum = 0.f, l1_sum = 0.f;
    const int rows = min(SH, L.H - r0), n_end = rows + 4 * R;
    fetch(r0 - 2 * R);
    stage(0);
    fetch(r0 - 2 * R + 1);
    __syncthreads();

    // Step n, ring phase P = n mod 11: the image row i = r0 - 10 + n enters (H1, V1, P -> adjoint row i - 5), and the
    // adjoint row of step n - 1 goes through H2, V2 -> gradient row i - 11.  One step past the last image row drains it.
    auto step = [&](auto phase, int n) {
        constexpr int P = decltype(phase)::value;
        const int i = r0 - 2 * R + n, buf = n & 1;
        const bool head = n < n_end, tail = n > 2 * R;  // uniform: is there an image row / an adjoint row for this step?
        const int o = i - 2 * R - 1;                    // the gradient row this step completes (n > 20)
        const bool emit = n > 4 * R && out_col;
        float xo = 0.f, yo = 0.f;
        if (emit) {  // in flight across the whole step
            xo = row_ptr(x, o)[co];
            yo = row_ptr(y, o)[co];
        }
#if GS_LOSS_WEIGHTED
        float mo = 0.f, mr = 0.f;  // the weights of the gradient row this step completes and of its moment row
        if (emit) mo = weight_at(o);
        if (head && n >= 2 * R) mr = weight_at(i - R);
#endif
        if (head) {
            stage(buf ^ 1);  // the image row of step n + 1 (fetched during step n - 1)
            fetch(i + 2);
        }
        f2 h01 = {0.f, 0.f}, h23 = {0.f, 0.f}, g01 = {0.f, 0.f};
        float h4 = 0.f, g2 = 0.f;
        if (head) {  // H1
            const f2 *sxy = &s_xy[buf][t];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const f2 ab = sxy[3 * k];
                const f2 w = f2{Wd.g[k], Wd.g[k]} * ab;
                h01 += w;
                h23 = pfma(w, ab, h23);
                h4 = fmaf(w.x, ab.y, h4);
            }
        }
        if (tail) {  // H2 of the adjoint row written by step n - 1
            const f2 *sd01 = &s_d01[buf ^ 1][t];
            const float *sd2 = &s_d2[buf ^ 1][t];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                g01 = pfma(f2{Wd.g[k], Wd.g[k]}, sd01[3 * k], g01);
                g2 = fmaf(Wd.g[k], sd2[3 * k], g2);
            }
        }
        if (head) {
            // V1: image row n adds tap k to the partial sum of moment row n - k (slot (n - k) mod 11)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int slot = (P - k + K) % K;
                const f2 gk = {Wd.g[k], Wd.g[k]};
                a1p[slot][0] = k == 0 ? gk * h01 : pfma(gk, h01, a1p[slot][0]);
                a1p[slot][1] = k == 0 ? gk * h23 : pfma(gk, h23, a1p[slot][1]);
                a1s[slot] = k == 0 ? Wd.g[0] * h4 : fmaf(Wd.g[k], h4, a1s[slot]);
            }
            if (n >= 2 * R) {  // uniform: moment row rho = i - 5 is complete
                constexpr int E = (P + 1) % K;
                const int rho = i - R;
                const float mu = a1p[E][0].x, nu = a1p[E][0].y, exx = a1p[E][1].x, eyy = a1p[E][1].y, exy = a1s[E];
                const float vx_raw = exx - mu * mu, vy_raw = eyy - nu * nu;
                const float vx = fmaxf(vx_raw, 0.f), vy = fmaxf(vy_raw, 0.f);
                const float A1 = 2.f * mu * nu + L.c1, A2 = 2.f * (exy - mu * nu) + L.c2;
                const float B1 = mu * mu + nu * nu + L.c1, B2 = vx + vy + L.c2;
                // the three quotients through v_rcp_f32 (1 ulp) instead of IEEE divisions
                const float i1 = gs_rcp(B1), i2 = gs_rcp(B2), inv = i1 * i2;
                const float S = A1 * A2 * inv, S_B2 = S * i2, S_B1 = S * i1;
                // dS/dExx = -S/B2 (zero where the variance clamp is active); the same factor enters dS/dmu
                const float dExx = vx_raw > 0.f ? -S_B2 : 0.f;
                const float dmu = 2.f * nu * (A2 - A1) * inv - 2.f * mu * S_B1 - 2.f * mu * dExx;
                const float dExy = 2.f * A1 * inv;
#if GS_LOSS_WEIGHTED
                // (a pixel of weight zero is no interior pixel: its adjoints are +0.0 whatever S is there)
                const bool valid = col_in && rho >= R && rho < L.H - R && mr > 0.f;
                if (valid && out_col && rho >= r0 && rho < r0 + SH) ssim_sum += mr * S;
                s_d01[buf][t + FHALO] = f2{valid ? mr * dmu : 0.f, valid ? mr * dExx : 0.f};
                s_d2[buf][t + FHALO] = valid ? mr * dExy : 0.f;
#else
                const bool valid = col_in && rho >= R && rho < L.H - R;  // the window lies inside the image
                if (valid && out_col && rho >= r0 && rho < r0 + SH) ssim_sum += S;
                s_d01[buf][t + FHALO] = f2{valid ? dmu : 0.f, valid ? dExx : 0.f};
                s_d2[buf][t + FHALO] = valid ? dExy : 0.f;
#endif
            }
        }
        if (tail) {
            // V2: the adjoint row of step n - 1 was that step's phase P - 1, i.e. phase P of the second ring
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int slot = (P - k + K) % K;
                const f2 gk = {Wd.g[k], Wd.g[k]};
                a2p[slot] = k == 0 ? gk * g01 : pfma(gk, g01, a2p[slot]);
                a2s[slot] = k == 0 ? Wd.g[0] * g2 : fmaf(Wd.g[k], g2, a2s[slot]);
            }
            if (emit) {
                constexpr int E2 = (P + 1) % K;
                const float d = xo - yo;
#if GS_LOSS_WEIGHTED
                l1_sum += mo * fabsf(d);
                // the same product-minus-product as below, so that the compiler contracts it the same way (the first product
                // is exact there: +-a or 0); the sign picks +m or -m, and a zero weight gives +0.0 whatever the sign
                float g = L.a * (mo > 0.f ? (d > 0.f ? mo : d < 0.f ? -mo : 0.f) : 0.f);
#else
                l1_sum += fabsf(d);
                float g = L.a * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);  // torch: sign(0) = 0
#endif
                g -= L.b * (a2p[E2].x + 2.f * xo * a2p[E2].y + yo * a2s[E2]);
                grad[(size_t)o * F + cv] = g;
            }
        }
        __syncthreads();
    };
    for (int nb = 0; nb <= n_end; nb += K) {
#define GS_LOSS_STEP(PH) \
    if (nb + PH <= n_end) step(std::integral_constant<int, PH>{}, nb + PH);
        GS_LOSS_STEP(0)
        GS_LOSS_STEP(1)
        GS_LOSS_STEP(2)
        GS_LOSS_STEP(3)
        GS_LOSS_STEP(4)
        GS_LOSS_STEP(5)
        GS_LOSS_STEP(6)
        GS_LOSS_STEP(7)
        GS_LOSS_STEP(8)
        GS_LOSS_STEP(9)
        GS_LOSS_STEP(10)
#undef GS_LOSS_STEP
    }
    __syncthreads();
    const float tot_s = block_sum<FT / 64>(ssim_sum, s_red);
    __syncthreads();
    const float tot_l = block_sum<FT / 64>(l1_sum, s_red);
    if (t == 0) {
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
        p_ssim[blk] = tot_s;
        p_l1[blk] = tot_l;
    }
