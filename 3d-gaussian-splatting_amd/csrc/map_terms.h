// map_terms.h -- the per-pixel terms the losses on a GS_FRAME_AUX frame's maps share (map_loss.hip: gs_loss_depth,
// gs_loss_track; track_gate.hip: gs_loss_track_gated).  Every includer is compiled with -ffp-contract=off: one rounding per
// operation, so the same pixel gives the same bits in every kernel that states it through these.
#pragma once
#include "gs_common.h"

#ifdef __HIPCC__

__device__ __forceinline__ bool map_measured(float z) { return z > 0.f && z <= 3.402823466e38f; }  // (false for NaN and +inf)

__device__ __forceinline__ float map_signed(float d, float s) { return d > 0.f ? s : (d < 0.f ? -s : 0.f); }

// the expected-depth term, in two steps (tracking gates on |r| between them): e = D / A and the residual r = e - z; then,
// with sg = map_signed(r, .), the gradients sg dr/dD = sg (1 / A) and sg dr/dA = sg (-(e / A)).  A > 0.
__device__ __forceinline__ float map_expected_residual(float D, float A, float z, float &e) {
    e = D / A;
    return e - z;
}
__device__ __forceinline__ void map_expected_grads(float sg, float e, float A, float &gD, float &gA) {
    gD = sg * (1.f / A);
    gA = sg * (-(e / A));
}

#endif  // __HIPCC__
