// overlap_count_body.inc -- the body of overlap_count_kernel and of overlap_count_pp_kernel (overlap.hip), expanded in place
// in both.  Expects in scope: the kernels' parameters, `constexpr bool PP` and -- PP -- cam_dx, cam_dy, view_pp.  (Included
// rather than called: expanded in place, the kernel of a call without offsets compiles to the code it had before the
// variant existed.)
    __shared__ uint32_t s_cnt[OVL_WAVES][GS_OVERLAP_MAX_VIEWS + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t acc[OVL_GROUPS] = {0, 0, 0, 0};
    uint32_t n_meas = 0, n_none = 0;  // (the same in every lane of the wave)
    const int64_t chunk0 = (int64_t)blockIdx.x * G.chunks_per_block;
    for (int32_t c = 0; c < G.chunks_per_block; ++c) {
        const int64_t base = (chunk0 + c) * OVL_BLOCK;
        if (base >= G.L) break;
        const int64_t j = base + threadIdx.x;
        bool meas = false;
        float p[3] = {0.f, 0.f, 0.f};
        if (j < G.L) {
            const int32_t ly = (int32_t)(j / G.Lw), lx = (int32_t)(j - (int64_t)ly * G.Lw);
            const int32_t x = lx * G.stride + G.off, y = ly * G.stride + G.off;
            const float z = range[(int64_t)y * G.W + x];
            meas = gs_overlap_measured(z);
            if (meas) {
                if (PP) gs_overlap_point_pp(cam, cam_dx, cam_dy, x, y, z, p);
                else gs_overlap_point(cam, x, y, z, p);
            }
        }
        const unsigned long long mm = __ballot(meas);
        if (mm == 0ull) continue;  // (the whole wave alike)
        bool any = false;
#pragma unroll
        for (int g = 0; g < OVL_GROUPS; ++g) {
            const int kend = min(64, n_views - 64 * g);
            uint32_t a = acc[g];
            for (int kk = 0; kk < kend; ++kk) {
                bool seen;
                if (PP) {
                    const float2 d = view_pp ? view_pp[64 * g + kk] : make_float2(0.f, 0.f);
                    seen = meas & gs_overlap_seen_pp(p, views[64 * g + kk], d.x, d.y, near, border);
                } else {
                    seen = meas & gs_overlap_seen(p, views[64 * g + kk], near, border);
                }
                const uint32_t cnt = (uint32_t)__popcll(__ballot(seen));
                any = any || seen;
                a += lane == kk ? cnt : 0u;
            }
            acc[g] = a;
        }
        n_meas += (uint32_t)__popcll(mm);
        n_none += (uint32_t)__popcll(__ballot(meas && !any));
    }
#pragma unroll
    for (int g = 0; g < OVL_GROUPS; ++g) s_cnt[wave][64 * g + lane] = acc[g];
    if (lane == 0) {
        s_cnt[wave][GS_OVERLAP_MAX_VIEWS] = n_meas;
        s_cnt[wave][GS_OVERLAP_MAX_VIEWS + 1] = n_none;
    }
    __syncthreads();
    uint32_t *row = rows + (size_t)blockIdx.x * (size_t)(n_views + 2);
    for (int e = threadIdx.x; e < n_views + 2; e += OVL_BLOCK) {
        const int s = e < n_views ? e : GS_OVERLAP_MAX_VIEWS + (e - n_views);
        row[e] = s_cnt[0][s] + s_cnt[1][s] + s_cnt[2][s] + s_cnt[3][s];
    }
