// pose_step.hip -- the pose of a tracked frame, stepped on the device (gs_pose_step, gs_pose_reset, gs_pose_log_bytes;
// include/gs_abi.h).
//
// gs_track.PoseAdam.step, so3_exp, rot_tangent_grad and the best-pose bookkeeping of Tracker.track, restated in double with
// explicit scalar operations: every sum runs left to right, every product is rounded before it is added (the file is built
// with -ffp-contract=off), so tests/pose_step_ref.py -- the same statements in Python floats -- follows it operation by
// operation.  What may differ from the host in the last bit are sqrt, sin, cos and pow alone.
//   pose_step_kernel  : ONE wave.  Every lane reads the skip flag; lane k < 24 + n_values reads element k of the log row (pose,
//                       gradients, values) and stores it -- a plain store per lane.  Lane 0 then takes the step on the state
//                       and stores the new state and the 12 floats of pose_dev.  No atomics; a pure function of its inputs.
//                       A launch-latency kernel: nothing here is tuned.
//   pose_reset_kernel : zeroes the log, lane 0 of workgroup 0 writes the state and pose_dev.
#include <cmath>

#include "gs_common.h"

namespace {

static_assert(sizeof(gs_pose_state) == 37 * 8 + 4 * 4, "the device state is 37 doubles and four int32");
static_assert(GS_POSE_LOG_HEAD == 24, "log row: 12 pose floats, 12 gradient floats, then the loss's values");

struct PoseStepArgs {
    double lr[6], b1, b2, eps;
    int32_t track_best, n_values, log_row, pad;
};

__device__ __forceinline__ bool pose_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (false for NaN)

__global__ void __launch_bounds__(64)
    pose_step_kernel(const float *__restrict__ grad_rot, const float *__restrict__ grad_tran, const float *__restrict__ values,
                     const unsigned long long *__restrict__ skip_if_nonzero, PoseStepArgs a, gs_pose_state *__restrict__ state,
                     float *pose_dev, float *__restrict__ log_row) {
    const int lane = (int)threadIdx.x;
    const bool skip = skip_if_nonzero != nullptr && *skip_if_nonzero != 0ull;
    // the log row: what the frame just rendered (pose_dev before this step), its gradients, its loss values
    const int row_len = GS_POSE_LOG_HEAD + a.n_values;
    if (lane < row_len) {
        float x = lane < 12 ? pose_dev[lane] : lane < 21 ? grad_rot[lane - 12] : lane < 24 ? grad_tran[lane - 21] : values[lane - 24];
        if (skip && lane == GS_POSE_LOG_HEAD) x = __builtin_nanf("");
        log_row[lane] = x;
    }
    __syncthreads();  // (the row's pose has been read by its lanes before lane 0 replaces it)
    if (lane != 0) return;
    if (skip) {
        state->skipped += 1;
        return;
    }
    double G[9], g[6];
    bool ok = pose_finite(values[0]);
    for (int k = 0; k < 9; ++k) {
        ok = ok && pose_finite(grad_rot[k]);
        G[k] = (double)grad_rot[k];
    }
    for (int k = 0; k < 3; ++k) {
        ok = ok && pose_finite(grad_tran[k]);
        g[3 + k] = (double)grad_tran[k];
    }
    if (!ok) {
        state->bad += 1;
        return;
    }
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = state->R[k];
    for (int k = 0; k < 3; ++k) t[k] = state->t[k];
    const double loss = (double)values[0];
    if (a.track_best && loss < state->best_loss) {  // the pose BEFORE the step: the one this loss belongs to
        for (int k = 0; k < 9; ++k) state->best_R[k] = R[k];
        for (int k = 0; k < 3; ++k) state->best_t[k] = t[k];
        state->best_loss = loss;
        state->best_row = a.log_row;
    }
    // dL/dw at w = 0 of exp([w]x) R: M = G R^T, (M21 - M12, M02 - M20, M10 - M01)
    double M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = G[3 * i] * R[3 * j] + G[3 * i + 1] * R[3 * j + 1] + G[3 * i + 2] * R[3 * j + 2];
    g[0] = M[7] - M[5];
    g[1] = M[2] - M[6];
    g[2] = M[3] - M[1];
    const int steps = state->steps + 1;
    state->steps = steps;
    const double bc1 = 1.0 - pow(a.b1, (double)steps), bc2 = 1.0 - pow(a.b2, (double)steps);
    double d[6];
    for (int k = 0; k < 6; ++k) {
        const double m = a.b1 * state->m[k] + (1.0 - a.b1) * g[k];
        const double v = a.b2 * state->v[k] + ((1.0 - a.b2) * g[k]) * g[k];
        state->m[k] = m;
        state->v[k] = v;
        d[k] = (a.lr[k] * (m / bc1)) / (sqrt(v / bc2) + a.eps);
    }
    // E = exp([w]x), w = -d[0:3] (Rodrigues; the series below 1e-8 rad)
    const double w0 = -d[0], w1 = -d[1], w2 = -d[2];
    const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    double KK[9], E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) KK[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    double ca = 1.0, cb = 0.5;
    if (!(th < 1e-8)) {
        ca = sin(th) / th;
        cb = (1.0 - cos(th)) / (th * th);
    }
    for (int k = 0; k < 9; ++k) E[k] = ((k % 4 == 0 ? 1.0 : 0.0) + ca * K[k]) + cb * KK[k];
    double Rn[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
    for (int k = 0; k < 9; ++k) {
        state->R[k] = Rn[k];
        pose_dev[k] = (float)Rn[k];
    }
    for (int k = 0; k < 3; ++k) {
        const double tn = t[k] - d[3 + k];
        state->t[k] = tn;
        pose_dev[9 + k] = (float)tn;
    }
}

__global__ void __launch_bounds__(256)
    pose_reset_kernel(gs_pose_state init, gs_pose_state *__restrict__ state, float *__restrict__ pose_dev, float *__restrict__ log,
                      int64_t n_log) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_log) log[i] = 0.f;
    if (i == 0) {
        *state = init;
        for (int k = 0; k < 9; ++k) pose_dev[k] = (float)init.R[k];
        for (int k = 0; k < 3; ++k) pose_dev[9 + k] = (float)init.t[k];
    }
}

bool pose_positive(double x) { return x > 0.0 && std::isfinite(x); }

}  // namespace

extern "C" size_t gs_pose_log_bytes(int32_t rows, int32_t n_values) {
    if (rows < 1 || (n_values != 4 && n_values != 8)) return 0;
    return sizeof(float) * (size_t)(GS_POSE_LOG_HEAD + n_values) * (size_t)rows;
}

extern "C" int gs_pose_reset(gs_pose_state *state_dev, float *pose_dev, float *log_dev, int32_t log_rows, int32_t n_values,
                             const double *rot, const double *tran, gs_stream_t stream) {
    GS_CHECK_ARG(state_dev != nullptr && pose_dev != nullptr && log_dev != nullptr, "state_dev, pose_dev or log_dev is null");
    GS_CHECK_ARG(rot != nullptr && tran != nullptr, "rot or tran is null");
    GS_CHECK_ARG(((uintptr_t)state_dev & 7) == 0, "state_dev must be 8-byte aligned");
    GS_CHECK_ARG((((uintptr_t)pose_dev | (uintptr_t)log_dev) & 15) == 0, "pose_dev and log_dev must be 16-byte aligned");
    GS_CHECK_ARG(n_values == 4 || n_values == 8, "n_values must be 4 or 8");
    GS_CHECK_ARG(log_rows >= 1, "log_rows must be >= 1");
    gs_pose_state init = {};
    for (int k = 0; k < 9; ++k) {
        GS_CHECK_ARG(std::isfinite(rot[k]), "rot must be finite");
        init.R[k] = init.best_R[k] = rot[k];
    }
    for (int k = 0; k < 3; ++k) {
        GS_CHECK_ARG(std::isfinite(tran[k]), "tran must be finite");
        init.t[k] = init.best_t[k] = tran[k];
    }
    init.best_loss = INFINITY;
    init.best_row = -1;
    const int64_t n_log = (int64_t)log_rows * (GS_POSE_LOG_HEAD + n_values);
    hipLaunchKernelGGL(pose_reset_kernel, dim3((unsigned)gs_div_up(n_log, 256)), dim3(256), 0, (hipStream_t)stream, init,
                       state_dev, pose_dev, log_dev, n_log);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_pose_step(const float *grad_rot_dev, const float *grad_tran_dev, const float *values_dev,
                            const void *skip_if_nonzero, const gs_pose_step_opts *opts, gs_pose_state *state_dev,
                            float *pose_dev, float *log_dev, int32_t log_rows, int32_t log_row, gs_stream_t stream) {
    GS_CHECK_ARG(grad_rot_dev != nullptr && grad_tran_dev != nullptr && values_dev != nullptr,
                 "grad_rot_dev, grad_tran_dev or values_dev is null");
    GS_CHECK_ARG(opts != nullptr, "opts is null");
    GS_CHECK_ARG(state_dev != nullptr && pose_dev != nullptr && log_dev != nullptr, "state_dev, pose_dev or log_dev is null");
    GS_CHECK_ARG(pose_positive(opts->lr_rot) && pose_positive(opts->lr_tran) && pose_positive(opts->lr_scale),
                 "lr_rot, lr_tran and lr_scale must be positive and finite");
    GS_CHECK_ARG(pose_positive(opts->eps), "eps must be positive and finite");
    GS_CHECK_ARG(opts->beta1 >= 0.0 && opts->beta1 < 1.0 && opts->beta2 >= 0.0 && opts->beta2 < 1.0, "betas must lie in [0, 1)");
    GS_CHECK_ARG(opts->n_values == 4 || opts->n_values == 8, "n_values must be 4 or 8");
    GS_CHECK_ARG(log_rows >= 1 && log_row >= 0 && log_row < log_rows, "log_row must lie in [0, log_rows)");
    GS_CHECK_ARG((((uintptr_t)state_dev | (uintptr_t)skip_if_nonzero) & 7) == 0, "state_dev and skip_if_nonzero must be 8-byte aligned");
    GS_CHECK_ARG((((uintptr_t)pose_dev | (uintptr_t)log_dev) & 15) == 0, "pose_dev and log_dev must be 16-byte aligned");
    GS_CHECK_ARG((((uintptr_t)grad_rot_dev | (uintptr_t)grad_tran_dev | (uintptr_t)values_dev) & 3) == 0,
                 "grad_rot_dev, grad_tran_dev and values_dev must be 4-byte aligned");
    PoseStepArgs a;
    for (int k = 0; k < 6; ++k) a.lr[k] = (k < 3 ? opts->lr_rot : opts->lr_tran) * opts->lr_scale;
    a.b1 = opts->beta1;
    a.b2 = opts->beta2;
    a.eps = opts->eps;
    a.track_best = opts->track_best != 0;
    a.n_values = opts->n_values;
    a.log_row = log_row;
    a.pad = 0;
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, grad_rot_dev, grad_tran_dev, values_dev,
                       (const unsigned long long *)skip_if_nonzero, a, state_dev, pose_dev,
                       log_dev + (size_t)log_row * (GS_POSE_LOG_HEAD + opts->n_values));
    GS_CHECK_LAUNCH();
    return 0;
}
