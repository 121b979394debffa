// icp.hip -- frame-to-model point-to-plane ICP on the device (gs_icp_model_maps, gs_icp_step, gs_icp_reset; include/gs_abi.h).
//
// icp_point.h states the arithmetic of one pixel; this file runs it over images and solves.
//   M  icp_model_kernel    : a thread per model pixel, 256 per workgroup, NO grid cap (an image of 2^31 pixels or more is
//                            refused): the pixel's range and its four stencil neighbours' -> one float4 vertex and one float4
//                            normal, 16-byte stores.  Every pixel of both maps is written: the maps are a pure function of
//                            the inputs.
//   S1 icp_accum_kernel    : a 256-thread workgroup takes a run of consecutive lattice pixels in row-major order, 256 at a
//                            time, a thread per pixel (overlap.hip's lattice and plan).  A thread back-projects its pixel,
//                            moves it by the state (read from device memory, rounded to fp32 once), gathers the model pixel it
//                            falls on -- two 16-byte loads, the only irregular access -- and adds its 28 terms to 28
//                            registers, one term per chunk of its workgroup's run: m = chunks_per_block sequential adds.
//                            Then a butterfly over the wave's 64 lanes (xor 32, 16, ..., 1: every lane ends with the same sum,
//                            in an order fixed by the lane numbers), the four waves' sums meet in LDS and are added in wave
//                            order.  Kept and measured pixels are counted by ballot.  The workgroup writes one 32-float row:
//                            28 sums, the two counts as uint32, two zeros.  The grid is capped at ICP_MAX_BLOCKS workgroups;
//                            beyond 262,144 lattice pixels a workgroup's run holds several chunks.
//   S2 icp_solve_kernel    : ONE workgroup.  Thread t adds rows t, t + 256, ... in ascending order in double (counts in
//                            int64), the 256 partial sums of a column are added in thread order by one thread per column;
//                            thread 0 then solves (A + damping tr(A) / 6 I) x = -b by Cholesky in double, applies
//                            R <- exp([x_w]x) R, t <- exp([x_w]x) t + x_t to the device state and writes the log row.
//                            With fewer than min_count kept pixels, or a pivot that is not positive, the state's pose stays
//                            bit for bit and the status says so; the iteration counter advances either way.
// No atomics, no host synchronisation; every row S2 reads was written whole by S1 in the same call, and the fixed orders above
// make the result a pure function of the inputs whatever the workspace held.  Every store is a vector store or plain C++.
#include <cmath>

#include "gs_common.h"
#include "icp_point.h"

namespace {

constexpr int ICP_BLOCK = 256, ICP_WAVES = ICP_BLOCK / 64;
constexpr int ICP_MAX_BLOCKS = 1024;  // four workgroups on each of 256 CUs: longer runs beyond that
constexpr int ICP_ROW = 32;           // floats per workspace row: 28 sums, kept, measured (uint32), two zeros
constexpr int ICP_COLS = GS_ICP_TERMS + 2;
static_assert(sizeof(gs_icp_state) == 104, "the device state is 12 doubles and two int32");
static_assert(GS_ICP_LOG_DOUBLES == 3 + GS_ICP_TERMS - 1 + 6 + 2 + 2, "log row: counts, e e, 27 sums, x, status, damping, pad");

struct IcpLattice {
    int32_t W, stride, off, Lw;
    int64_t L;
    int32_t chunks_per_block;
};

struct IcpPlan {
    IcpLattice G;
    int32_t nblk;  // workgroups of S1 = rows of the workspace
};

inline IcpPlan icp_plan(int32_t H, int32_t W, int32_t stride) {
    IcpPlan P;
    IcpLattice &G = P.G;
    G.W = W;
    G.stride = stride;
    G.off = stride / 2;
    G.Lw = W > G.off ? (W - G.off + stride - 1) / stride : 0;
    const int32_t Lh = H > G.off ? (H - G.off + stride - 1) / stride : 0;
    G.L = (int64_t)G.Lw * Lh;
    const int64_t chunks = gs_div_up(G.L, ICP_BLOCK);
    G.chunks_per_block = (int32_t)(chunks > ICP_MAX_BLOCKS ? gs_div_up(chunks, ICP_MAX_BLOCKS) : 1);
    P.nblk = (int32_t)gs_div_up(chunks, G.chunks_per_block);
    return P;
}

__global__ void __launch_bounds__(ICP_BLOCK)
    icp_model_kernel(const float *__restrict__ depth, const float *__restrict__ alpha, gs_icp_cam cam, float alpha_min,
                     float edge_rel, float one_plus, int32_t step, float4 *__restrict__ vertex, float4 *__restrict__ normal) {
    const int64_t at = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (at >= (int64_t)cam.W * cam.H) return;
    const int32_t y = (int32_t)(at / cam.W), x = (int32_t)(at - (int64_t)y * cam.W);
    float v[4], n[4];
    gs_icp_model_pixel(depth, alpha, cam, x, y, alpha_min, edge_rel, one_plus, step, v, n);
    vertex[at] = make_float4(v[0], v[1], v[2], v[3]);
    normal[at] = make_float4(n[0], n[1], n[2], n[3]);
}

__global__ void __launch_bounds__(ICP_BLOCK)
    icp_accum_kernel(const float *__restrict__ range, IcpLattice G, gs_icp_cam cam, const float4 *__restrict__ vertex,
                     const float4 *__restrict__ normal, gs_icp_cam model, float dist_max, float cos_min,
                     const gs_icp_state *__restrict__ state, float *__restrict__ rows) {
    __shared__ float s_sum[ICP_WAVES][GS_ICP_TERMS];
    __shared__ uint32_t s_cnt[ICP_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rt[k] = (float)state->R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Rt[9 + k] = (float)state->t[k];
    float acc[GS_ICP_TERMS];
#pragma unroll
    for (int k = 0; k < GS_ICP_TERMS; ++k) acc[k] = 0.f;
    uint32_t kept = 0, measured = 0;  // (wave-uniform: popcounts of ballots)
    const int64_t first = (int64_t)blockIdx.x * G.chunks_per_block * ICP_BLOCK;
    for (int32_t c = 0; c < G.chunks_per_block; ++c) {
        const int64_t l = first + (int64_t)c * ICP_BLOCK + threadIdx.x;
        bool has = false, keep = false;
        float term[GS_ICP_TERMS];
        if (l < G.L) {
            const int32_t ly = (int32_t)(l / G.Lw), lx = (int32_t)(l - (int64_t)ly * G.Lw);
            const int32_t x = lx * G.stride + G.off, y = ly * G.stride + G.off;
            const float z = range[(int64_t)y * G.W + x];
            has = gs_icp_measured(z);
            if (has) {
                float p[3], q[3];
                gs_icp_point(cam, x, y, z, p);
                gs_icp_transform(Rt, p, q);
                const int64_t at = gs_icp_project(model, q);  // (inside the model image or -1)
                if (at >= 0) {
                    const float4 n4 = normal[at], v4 = vertex[at];
                    const float v[4] = {v4.x, v4.y, v4.z, v4.w}, n[4] = {n4.x, n4.y, n4.z, n4.w};
                    keep = gs_icp_terms(q, v, n, dist_max, cos_min, term);
                }
            }
        }
        if (keep) {
#pragma unroll
            for (int k = 0; k < GS_ICP_TERMS; ++k) acc[k] += term[k];
        }
        measured += (uint32_t)__popcll(__ballot(has));
        kept += (uint32_t)__popcll(__ballot(keep));
    }
#pragma unroll
    for (int k = 0; k < GS_ICP_TERMS; ++k) {
        float s = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        acc[k] = s;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < GS_ICP_TERMS; ++k) s_sum[wave][k] = acc[k];
        s_cnt[wave][0] = kept;
        s_cnt[wave][1] = measured;
    }
    __syncthreads();
    float *row = rows + (size_t)blockIdx.x * ICP_ROW;
    const int t = threadIdx.x;
    if (t < GS_ICP_TERMS) {
        row[t] = ((s_sum[0][t] + s_sum[1][t]) + s_sum[2][t]) + s_sum[3][t];
    } else if (t < ICP_COLS) {
        const int k = t - GS_ICP_TERMS;
        reinterpret_cast<uint32_t *>(row)[t] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
    } else if (t < ICP_ROW) {
        row[t] = 0.f;
    }
}

// exp([w]x) in double (Rodrigues; the series below 1e-8 rad, as gs_track.so3_exp)
__device__ void icp_so3_exp(const double w[3], double E[9]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a = 1.0, b = 0.5;
    if (th >= 1e-8) {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int m = 0; m < 3; ++m) kk += K[3 * i + m] * K[3 * m + j];
            E[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K[3 * i + j] + b * kk;
        }
}

__global__ void __launch_bounds__(ICP_BLOCK)
    icp_solve_kernel(const float *__restrict__ rows, int32_t nblk, double damping, int32_t min_count, int32_t stride,
                     gs_icp_state *__restrict__ state, double *__restrict__ log_row) {
    __shared__ double s_part[ICP_COLS][ICP_BLOCK];
    __shared__ double s_tot[ICP_COLS];
    const int t = threadIdx.x;
    {
        double sum[GS_ICP_TERMS];
        long long cnt[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < GS_ICP_TERMS; ++k) sum[k] = 0.0;
        for (int32_t r = t; r < nblk; r += ICP_BLOCK) {
            const float4 *row = reinterpret_cast<const float4 *>(rows + (size_t)r * ICP_ROW);
#pragma unroll
            for (int k4 = 0; k4 < GS_ICP_TERMS / 4; ++k4) {
                const float4 f = row[k4];
                sum[4 * k4] += (double)f.x, sum[4 * k4 + 1] += (double)f.y;
                sum[4 * k4 + 2] += (double)f.z, sum[4 * k4 + 3] += (double)f.w;
            }
            const float4 f = row[GS_ICP_TERMS / 4];
            cnt[0] += (long long)__float_as_uint(f.x);
            cnt[1] += (long long)__float_as_uint(f.y);
        }
#pragma unroll
        for (int k = 0; k < GS_ICP_TERMS; ++k) s_part[k][t] = sum[k];
        s_part[GS_ICP_TERMS][t] = (double)cnt[0];      // (exact: a count stays far below 2^53)
        s_part[GS_ICP_TERMS + 1][t] = (double)cnt[1];
    }
    __syncthreads();
    if (t < ICP_COLS) {
        double s = 0.0;
        for (int k = 0; k < ICP_BLOCK; ++k) s += s_part[t][k];
        s_tot[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    const double kept = s_tot[GS_ICP_TERMS], measured = s_tot[GS_ICP_TERMS + 1];
    double A[6][6], b[6], x[6] = {0, 0, 0, 0, 0, 0};
    {
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s_tot[k++];
        for (int i = 0; i < 6; ++i) b[i] = s_tot[k++];
    }
    const double lambda = damping * (A[0][0] + A[1][1] + A[2][2] + A[3][3] + A[4][4] + A[5][5]) / 6.0;
    int status = GS_ICP_OK;
    if (kept < (double)min_count) {
        status = GS_ICP_TOO_FEW;
    } else {
        double Lc[6][6];
        for (int j = 0; j < 6 && status == GS_ICP_OK; ++j) {
            double d = A[j][j] + lambda;
            for (int k = 0; k < j; ++k) d -= Lc[j][k] * Lc[j][k];
            if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) {
                status = GS_ICP_NOT_POSITIVE;
                break;
            }
            Lc[j][j] = sqrt(d);
            for (int i = j + 1; i < 6; ++i) {
                double s = A[i][j];
                for (int k = 0; k < j; ++k) s -= Lc[i][k] * Lc[j][k];
                Lc[i][j] = s / Lc[j][j];
            }
        }
        if (status == GS_ICP_OK) {
            double yv[6];
            for (int i = 0; i < 6; ++i) {
                double s = -b[i];
                for (int k = 0; k < i; ++k) s -= Lc[i][k] * yv[k];
                yv[i] = s / Lc[i][i];
            }
            for (int i = 5; i >= 0; --i) {
                double s = yv[i];
                for (int k = i + 1; k < 6; ++k) s -= Lc[k][i] * x[k];
                x[i] = s / Lc[i][i];
            }
            for (int i = 0; i < 6; ++i)
                if (!(fabs(x[i]) <= 1.7976931348623157e308)) status = GS_ICP_NOT_POSITIVE;  // (NaN or inf sums)
            if (status != GS_ICP_OK)
                for (int i = 0; i < 6; ++i) x[i] = 0.0;
        }
    }
    if (status == GS_ICP_OK) {
        double E[9], R[9], tt[3];
        icp_so3_exp(x, E);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j)
                R[3 * i + j] = E[3 * i] * state->R[j] + E[3 * i + 1] * state->R[3 + j] + E[3 * i + 2] * state->R[6 + j];
            tt[i] = E[3 * i] * state->t[0] + E[3 * i + 1] * state->t[1] + E[3 * i + 2] * state->t[2] + x[3 + i];
        }
        for (int k = 0; k < 9; ++k) state->R[k] = R[k];
        for (int k = 0; k < 3; ++k) state->t[k] = tt[k];
    }
    state->iteration += 1;
    log_row[0] = kept;
    log_row[1] = measured;
    log_row[2] = s_tot[GS_ICP_TERMS - 1];
    for (int k = 0; k < GS_ICP_TERMS - 1; ++k) log_row[3 + k] = s_tot[k];
    for (int k = 0; k < 6; ++k) log_row[30 + k] = x[k];
    log_row[36] = (double)status;
    log_row[37] = lambda;
    log_row[38] = (double)stride;
    log_row[39] = 0.0;
}

__global__ void __launch_bounds__(ICP_BLOCK)
    icp_reset_kernel(gs_icp_state init, gs_icp_state *__restrict__ state, double *__restrict__ log, int64_t n_log) {
    const int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i < n_log) log[i] = 0.0;
    if (i == 0) *state = init;
}

int icp_check_camera(const gs_seed_camera_pp *c, const char *null_text) {
    GS_CHECK_ARG(c != nullptr, null_text);
    GS_CHECK_ARG(c->cam.height > 0 && c->cam.width > 0 && (int64_t)c->cam.height * c->cam.width < (1ll << 31),
                 "image size out of range");
    GS_CHECK_ARG(c->cam.focal_x > 0.f && c->cam.focal_y > 0.f && std::isfinite(c->cam.focal_x) && std::isfinite(c->cam.focal_y),
                 "focal lengths must be positive and finite");
    GS_CHECK_ARG(std::isfinite(c->pp_dx) && std::isfinite(c->pp_dy), "the principal point's offset must be finite");
    return 0;
}

}  // namespace

extern "C" size_t gs_icp_model_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
    return sizeof(float4) * (size_t)H * (size_t)W;
}

extern "C" size_t gs_icp_workspace_bytes(int32_t H, int32_t W, int32_t stride) {
    if (H <= 0 || W <= 0 || stride < 1) return 0;
    const IcpPlan P = icp_plan(H, W, stride);
    return gs_align_up(sizeof(float) * ICP_ROW * (size_t)(P.nblk > 0 ? P.nblk : 1), 256);
}

extern "C" size_t gs_icp_log_bytes(int32_t rows) {
    if (rows < 1) return 0;
    return sizeof(double) * GS_ICP_LOG_DOUBLES * (size_t)rows;
}

extern "C" int gs_icp_model_maps(const float *depth, const float *alpha, const gs_seed_camera_pp *cam,
                                 const gs_icp_model_opts *opts, float *vertex, float *normal, gs_stream_t stream) {
    GS_CHECK_ARG(depth != nullptr, "depth is null");
    GS_CHECK_ARG(opts != nullptr, "opts is null");
    GS_CHECK_ARG(vertex != nullptr && normal != nullptr, "vertex or normal is null");
    int rc = icp_check_camera(cam, "camera is null");
    if (rc) return rc;
    GS_CHECK_ARG((((uintptr_t)vertex | (uintptr_t)normal) & 15) == 0, "vertex and normal must be 16-byte aligned");
    GS_CHECK_ARG(opts->normal_step >= 1, "normal_step must be >= 1");
    GS_CHECK_ARG(!std::isnan(opts->alpha_min), "alpha_min must not be NaN");
    GS_CHECK_ARG(!std::isnan(opts->edge_rel), "edge_rel must not be NaN (negative: the edge test is off)");
    const gs_icp_cam c = gs_icp_camera(*cam);
    const int64_t n = (int64_t)c.W * c.H;
    const float one_plus = 1.f + opts->edge_rel;
    hipLaunchKernelGGL(icp_model_kernel, dim3((unsigned)gs_div_up(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, (hipStream_t)stream, depth,
                       alpha, c, opts->alpha_min, opts->edge_rel, one_plus, opts->normal_step, (float4 *)vertex,
                       (float4 *)normal);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_icp_step(const float *range, const gs_seed_camera_pp *cam, const float *vertex, const float *normal,
                           const gs_seed_camera_pp *model_cam, const gs_icp_opts *opts, gs_icp_state *state_dev,
                           double *log_dev, int32_t log_rows, int32_t log_row, void *workspace, size_t workspace_bytes,
                           gs_stream_t stream) {
    GS_CHECK_ARG(range != nullptr, "range is null");
    GS_CHECK_ARG(vertex != nullptr && normal != nullptr, "vertex or normal is null");
    GS_CHECK_ARG(opts != nullptr, "opts is null");
    GS_CHECK_ARG(state_dev != nullptr && log_dev != nullptr, "state_dev or log_dev is null");
    int rc = icp_check_camera(cam, "camera is null");
    if (rc) return rc;
    rc = icp_check_camera(model_cam, "model camera is null");
    if (rc) return rc;
    GS_CHECK_ARG(opts->stride >= 1, "stride must be >= 1");
    GS_CHECK_ARG(opts->dist_max > 0.f, "dist_max must be positive (and not NaN)");
    GS_CHECK_ARG(!std::isnan(opts->cos_min), "cos_min must not be NaN");
    GS_CHECK_ARG(opts->damping >= 0.0 && std::isfinite(opts->damping), "damping must be finite and not negative");
    GS_CHECK_ARG(opts->min_count >= 0, "min_count must not be negative");
    GS_CHECK_ARG((((uintptr_t)vertex | (uintptr_t)normal) & 15) == 0, "vertex and normal must be 16-byte aligned");
    GS_CHECK_ARG((((uintptr_t)state_dev | (uintptr_t)log_dev) & 7) == 0, "state_dev and log_dev must be 8-byte aligned");
    GS_CHECK_ARG(log_rows >= 1 && log_row >= 0, "log_rows must be >= 1 and log_row >= 0");
    GS_CHECK_ARG(log_row < log_rows, "the log is full");
    GS_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0
                     && workspace_bytes >= gs_icp_workspace_bytes(cam->cam.height, cam->cam.width, opts->stride),
                 "workspace null, misaligned or too small");
    hipStream_t s = (hipStream_t)stream;
    const IcpPlan P = icp_plan(cam->cam.height, cam->cam.width, opts->stride);
    float *rows = (float *)workspace;
    if (P.nblk > 0) {
        hipLaunchKernelGGL(icp_accum_kernel, dim3(P.nblk), dim3(ICP_BLOCK), 0, s, range, P.G, gs_icp_camera(*cam),
                           (const float4 *)vertex, (const float4 *)normal, gs_icp_camera(*model_cam), opts->dist_max,
                           opts->cos_min, (const gs_icp_state *)state_dev, rows);
        GS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(ICP_BLOCK), 0, s, (const float *)rows, P.nblk, opts->damping,
                       opts->min_count, opts->stride, state_dev, log_dev + (size_t)log_row * GS_ICP_LOG_DOUBLES);
    GS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gs_icp_reset(gs_icp_state *state_dev, double *log_dev, int32_t log_rows, const double *rot, const double *tran,
                            gs_stream_t stream) {
    GS_CHECK_ARG(state_dev != nullptr && log_dev != nullptr, "state_dev or log_dev is null");
    GS_CHECK_ARG(rot != nullptr && tran != nullptr, "rot or tran is null");
    GS_CHECK_ARG((((uintptr_t)state_dev | (uintptr_t)log_dev) & 7) == 0, "state_dev and log_dev must be 8-byte aligned");
    GS_CHECK_ARG(log_rows >= 1, "log_rows must be >= 1");
    gs_icp_state init;
    for (int k = 0; k < 9; ++k) {
        GS_CHECK_ARG(std::isfinite(rot[k]), "rot must be finite");
        init.R[k] = rot[k];
    }
    for (int k = 0; k < 3; ++k) {
        GS_CHECK_ARG(std::isfinite(tran[k]), "tran must be finite");
        init.t[k] = tran[k];
    }
    init.iteration = 0;
    init.reserved = 0;
    const int64_t n_log = (int64_t)log_rows * GS_ICP_LOG_DOUBLES;
    hipLaunchKernelGGL(icp_reset_kernel, dim3((unsigned)gs_div_up(n_log, ICP_BLOCK)), dim3(ICP_BLOCK), 0, (hipStream_t)stream, init,
                       state_dev, log_dev, n_log);
    GS_CHECK_LAUNCH();
    return 0;
}
