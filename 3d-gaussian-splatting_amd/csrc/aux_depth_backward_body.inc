// aux_depth_backward_body.inc -- the body of frame_aux_depth_backward_kernel and of its GS_FRAME_POSE_GRAD variant
// frame_aux_depth_pose_backward_kernel (cull_project.hip), expanded in place in both (see frame_project_backward_body.inc).
// Expects in scope: the kernel's parameters, CDIM, `constexpr bool POSE` and, with POSE, `float pt[12]`.  Its `return`s
// leave the kernel -- or, in the pose variant, the lambda the body is expanded in.
    constexpr int RWF = gs_row_floats(CDIM), SLOT = gs_row_aux_depth(CDIM);
    const int64_t pid = g_first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= n) return;
    const uint4 rc = rects[pid];
    if (rc.z == 0) return;  // culled by the frustum test: zero gradient (written by the projection backward)
    const uint64_t off = pair_offsets[pid], cnt = rc.w;
    float gd = 0.f;
    if (CDIM != 3 && cnt > (uint64_t)GS_PB_SH_BIG) {
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
    float p[3], pc[3], gp[3];
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
        gp[c] = a;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_pos[pid * 3 + c] += gp[c];
    if constexpr (POSE) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pt[r * 3 + c] = gc[r] * p[c];
            pt[9 + r] = gc[r];
        }
    }
