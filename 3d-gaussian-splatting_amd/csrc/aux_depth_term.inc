// aux_depth_term.inc -- the depth map's position term of one visible Gaussian: g_d = the sum of the depth floats
// (gs_row_aux_depth) of its existing gradient rows in ascending order -- the first row alone beyond GS_PB_SH_BIG rows, where
// sh_big_rows_kernel has left the total --, gc = g_d p_c / |p_c| and gpa = rot^T gc, what enters dL/dpos.  Expanded in place
// in aux_depth_backward_body.inc (the kernels behind gs_frame_backward) and in the AUX variant of the fused optimizer step
// (frame_project_backward_body.inc): ONE statement of the row walk, so both add the same rows in the same order.
// Expects in scope: CDIM, P, D, pid, rc (the visible Gaussian's rectangle record), off, cnt, `const float *rows`, stop_keys,
// rec_geom, max_pairs, pos, GS_PB_SH_BIG (project_bwd.hip, in front of sh_big_rows_kernel), and `gd_known` / `gd_sum`: where
// gd_known holds, the caller has already added these rows in this order and g_d is gd_sum (the pose-only kernel's own row
// walk; everywhere else a constant false).  Leaves gd, p, pc, gc and gpa behind.
    constexpr int RWF = gs_row_floats(CDIM), SLOT = gs_row_aux_depth(CDIM);
    float gd = 0.f;
    if (gd_known) {
        gd = gd_sum;
    } else if (CDIM != 3 && cnt > (uint64_t)GS_PB_SH_BIG) {
        if (off < max_pairs) gd = rows[off * RWF + SLOT];
    } else {
        const uint32_t *stop_depth = reinterpret_cast<const uint32_t *>(stop_keys), *stop_id = stop_depth + P.ntx * P.nty;
        const uint32_t y0 = rc.x & 0xffff, x0 = rc.y & 0xffff, x1 = rc.y >> 16;
        float cx = 0.f, cy = 0.f;
        if (P.cull_method == 0) {
            const float4 g = rec_geom[pid * GS_REC_STRIDE];
            cx = g.x;
            cy = g.y;
        }
        uint32_t ix = x0, iy = y0;
        for (uint64_t k = 0; k < cnt && off + k < max_pairs; ++k) {
            const uint32_t t = iy * P.ntx + ix, sd = stop_depth[t];
            bool ex = rc.z < sd || (rc.z == sd && (uint32_t)pid <= stop_id[t]);
            if (P.cull_method == 0 && !gs_dist_listed(cx, cy, ix, iy, D)) ex = false;
            if (ex) gd += rows[(off + k) * RWF + SLOT];
            if (++ix == x1) {
                ix = x0;
                ++iy;
            }
        }
    }
    float p[3], pc[3], gpa[3];
    load3(pos, pid, p);
#pragma unroll
    for (int r = 0; r < 3; ++r)
        pc[r] = P.cam.rot[r * 3 + 0] * p[0] + P.cam.rot[r * 3 + 1] * p[1] + P.cam.rot[r * 3 + 2] * p[2] + P.cam.tran[r];
    const float ir_ = gs_rsq(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
    float gc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) gc[r] = gd * pc[r] * ir_;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float a = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) a += P.cam.rot[k * 3 + c] * gc[k];
        gpa[c] = a;
    }
