// aux_depth_backward_body.inc -- the body of frame_aux_depth_backward_kernel and of its GS_FRAME_POSE_GRAD variant
// frame_aux_depth_pose_backward_kernel (project_bwd.hip), expanded in place in both (see frame_project_backward_body.inc).
// Expects in scope: the kernel's parameters, CDIM, `constexpr bool POSE` and, with POSE, `float pt[12]`.  Its `return`s
// leave the kernel -- or, in the pose variant, the lambda the body is expanded in.  The row walk and the position term are
// aux_depth_term.inc, shared with the fused optimizer step's AUX variant.
    const int64_t pid = g_first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= n) return;
    const uint4 rc = rects[pid];
    if (rc.z == 0) return;  // culled by the frustum test: zero gradient (written by the projection backward)
    const uint64_t off = pair_offsets[pid], cnt = rc.w;
    constexpr bool gd_known = false;  // (the rows are walked here)
    constexpr float gd_sum = 0.f;
#include "aux_depth_term.inc"
#pragma unroll
    for (int c = 0; c < 3; ++c) grad_pos[pid * 3 + c] += gpa[c];
    if constexpr (POSE) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pt[r * 3 + c] = gc[r] * p[c];
            pt[9 + r] = gc[r];
        }
    }
