"""CPU tier of the depth alignment (include/gs_abi.h: gs_icp_model_maps, gs_icp_step, gs_icp_reset and the size queries;
csrc/icp_point.h; gs_icp): the symbols and bindings, every refusal on fake pointers (each comes before anything is enqueued),
the size queries, IcpOptions' validation, the pose algebra, the per-pixel header compiled for the host against the float32
restatement of tests/icp_ref.py, the float64 restatement on the analytic room corner -- the tracking criterion, and the slide
that is the documented reason for ``IcpResult.accepted`` -- and the trailing fields of gs_slam.  No kernel is launched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import icp_ref as R
from track_ref import perturbed_start, pose_errors, so3_exp_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splatting_amd", "csrc")
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 96, 128


def _cam(**kw):
    from gaussian import _lib

    c = _lib.GsSeedCameraPP()
    c.cam.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    c.cam.focal_x = c.cam.focal_y = 0.75 * W
    c.cam.width, c.cam.height = W, H
    for k, v in kw.items():
        setattr(c.cam if hasattr(c.cam, k) else c, k, v)
    return c


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    names = ("gs_icp_model_bytes", "gs_icp_workspace_bytes", "gs_icp_log_bytes", "gs_icp_model_maps", "gs_icp_reset",
             "gs_icp_step")
    for name in names:
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for text in ("size_t gs_icp_model_bytes(", "size_t gs_icp_workspace_bytes(", "size_t gs_icp_log_bytes(",
                 "int gs_icp_model_maps(", "int gs_icp_reset(", "int gs_icp_step(", "} gs_icp_model_opts;", "} gs_icp_opts;",
                 "} gs_icp_state;", "#define GS_ICP_LOG_DOUBLES 40", "e = n.(q - v),  J = (q x n, n)"):
        assert text in header, text
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    assert C.sizeof(_lib.GsIcpModelOpts) == 12 and C.sizeof(_lib.GsIcpOpts) == 24 and C.sizeof(_lib.GsIcpState) == 104
    assert _lib.GS_ICP_LOG_DOUBLES == 40 and (_lib.GS_ICP_OK, _lib.GS_ICP_TOO_FEW, _lib.GS_ICP_NOT_POSITIVE) == (0, 1, 2)
    point = open(os.path.join(CSRC, "icp_point.h")).read()
    assert "__host__ __device__" in point and "GS_ICP_TERMS 28" in point
    import gs_build

    assert "icp_point.h" in gs_build.HEADERS and "-ffp-contract=off" in gs_build.SOURCES["icp.hip"]


def test_size_queries():
    from gaussian import _lib

    sizes = [(1, 1), (37, 53), (120, 160), (480, 640), (1080, 1920), (2160, 3840)]
    model = [_lib.gs_icp_model_bytes(h, w) for h, w in sizes]
    assert model == [16 * h * w for h, w in sizes] and model == sorted(model)
    for stride in (1, 2, 4):
        got = [_lib.gs_icp_workspace_bytes(h, w, stride) for h, w in sizes]
        assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got) and got[-1] > got[0]  # monotone in the image
    for h, w in sizes:
        by_stride = [_lib.gs_icp_workspace_bytes(h, w, s) for s in (1, 2, 3, 8)]
        assert by_stride == sorted(by_stride, reverse=True)  # falling with the stride: fewer lattice pixels
    # a 128-byte row per workgroup of 256 lattice pixels, at most 1,024 workgroups: 640 x 480 takes runs of two chunks
    assert _lib.gs_icp_workspace_bytes(120, 160, 1) == 75 * 128 + 128  # (75 rows, rounded up to 256 bytes)
    assert _lib.gs_icp_workspace_bytes(480, 640, 1) == 600 * 128 + 0
    assert _lib.gs_icp_workspace_bytes(2160, 3840, 1) <= 1024 * 128
    logs = [_lib.gs_icp_log_bytes(n) for n in (1, 2, 19, 1000)]
    assert logs == [320 * n for n in (1, 2, 19, 1000)]
    for bad in ((0, 64), (48, -1), (1 << 16, 1 << 16)):
        assert _lib.gs_icp_model_bytes(*bad) == 0
    for bad in ((0, 64, 1), (48, 0, 1), (48, 64, 0), (48, 64, -2)):
        assert _lib.gs_icp_workspace_bytes(*bad) == 0
    assert _lib.gs_icp_log_bytes(0) == 0 and _lib.gs_icp_log_bytes(-3) == 0


def _refused(rc, word, what):
    from gaussian import _lib

    assert rc == GS_E_INVALID, what
    msg = _lib.gs_last_error()
    assert b"gs_icp" in msg or b"icp_check" in msg, msg
    assert word in msg, (what, msg)


def test_model_maps_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    D, A, V, N = (FAKE + i * (1 << 24) for i in range(4))

    def call(depth=D, alpha=A, cam="default", opts="default", vertex=V, normal=N):
        c = _cam() if cam == "default" else cam
        o = _lib.GsIcpModelOpts(0.5, 0.1, 1) if opts == "default" else opts
        return _lib.gs_icp_model_maps(depth, alpha, C.byref(c) if c is not None else None,
                                      C.byref(o) if o is not None else None, vertex, normal, None)

    for kw in ("depth", "cam", "opts", "vertex", "normal"):
        _refused(call(**{kw: None}), b"null", kw)
    for hw in (dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16)):
        _refused(call(cam=_cam(**hw)), b"size", hw)
    for f in (0.0, -2.0, float("nan"), float("inf")):
        _refused(call(cam=_cam(focal_x=f)), b"focal", f)
        _refused(call(cam=_cam(focal_y=f)), b"focal", f)
    for v in (float("nan"), float("inf"), -float("inf")):
        _refused(call(cam=_cam(pp_dx=v)), b"offset", v)
        _refused(call(cam=_cam(pp_dy=v)), b"offset", v)
    for s in (0, -1):
        _refused(call(opts=_lib.GsIcpModelOpts(0.5, 0.1, s)), b"normal_step", s)
    _refused(call(opts=_lib.GsIcpModelOpts(float("nan"), 0.1, 1)), b"alpha_min", "nan")
    _refused(call(opts=_lib.GsIcpModelOpts(0.5, float("nan"), 1)), b"edge_rel", "nan")
    _refused(call(vertex=V + 8), b"aligned", "vertex")
    _refused(call(normal=N + 4), b"aligned", "normal")


def test_step_and_reset_reject_bad_arguments_before_any_launch():
    from gaussian import _lib

    Z, V, N, S, L, WS = (FAKE + i * (1 << 24) for i in range(6))
    ws_bytes = _lib.gs_icp_workspace_bytes(H, W, 2)

    def opts(**kw):
        o = _lib.GsIcpOpts(2, 0.2, 0.0, 6, 1e-6)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(rng=Z, cam="default", vertex=V, normal=N, mcam="default", o="default", state=S, log=L, rows=19, row=0, ws=WS,
             nbytes=ws_bytes):
        c = _cam() if cam == "default" else cam
        m = _cam() if mcam == "default" else mcam
        o = opts() if o == "default" else o
        return _lib.gs_icp_step(rng, C.byref(c) if c is not None else None, vertex, normal,
                                C.byref(m) if m is not None else None, C.byref(o) if o is not None else None, state, log, rows,
                                row, ws, nbytes, None)

    for kw in ("rng", "cam", "vertex", "normal", "mcam", "o", "state", "log", "ws"):
        _refused(call(**{kw: None}), b"null", kw)
    for which in ("cam", "mcam"):
        for hw in (dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16)):
            _refused(call(**{which: _cam(**hw)}), b"size", (which, hw))
        for f in (0.0, -2.0, float("nan"), float("inf")):
            _refused(call(**{which: _cam(focal_x=f)}), b"focal", (which, f))
            _refused(call(**{which: _cam(focal_y=f)}), b"focal", (which, f))
        for v in (float("nan"), float("inf")):
            _refused(call(**{which: _cam(pp_dx=v)}), b"offset", (which, v))
            _refused(call(**{which: _cam(pp_dy=v)}), b"offset", (which, v))
    for s in (0, -1, -64):
        _refused(call(o=opts(stride=s)), b"stride", s)
    for v in (0.0, -0.2, float("nan")):
        _refused(call(o=opts(dist_max=v)), b"dist_max", v)
    _refused(call(o=opts(cos_min=float("nan"))), b"cos_min", "nan")
    for v in (-1e-6, float("nan"), float("inf")):
        _refused(call(o=opts(damping=v)), b"damping", v)
    _refused(call(o=opts(min_count=-1)), b"min_count", -1)
    _refused(call(vertex=V + 4), b"aligned", "vertex")
    _refused(call(state=S + 4), b"aligned", "state")
    _refused(call(log=L + 2), b"aligned", "log")
    _refused(call(ws=WS + 8), b"workspace", "misaligned")
    _refused(call(nbytes=ws_bytes - 1), b"workspace", "too small")
    _refused(call(o=opts(stride=1)), b"workspace", "sized for stride 2, asked for stride 1")
    _refused(call(row=19), b"full", "row == rows")
    _refused(call(row=40), b"full", "row > rows")
    _refused(call(row=-1), b"log_row", "negative")
    _refused(call(rows=0), b"log_rows", "no rows")

    eye, zero = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(0, 0, 0)

    def reset(state=S, log=L, rows=19, rot=eye, tran=zero):
        return _lib.gs_icp_reset(state, log, rows, rot, tran, None)

    for kw in ("state", "log", "rot", "tran"):
        _refused(reset(**{kw: None}), b"null", kw)
    _refused(reset(rows=0), b"log_rows", 0)
    _refused(reset(state=S + 4), b"aligned", "state")
    _refused(reset(rot=(C.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)), b"finite", "rot")
    _refused(reset(tran=(C.c_double * 3)(0, float("inf"), 0)), b"finite", "tran")


def test_options_are_validated():
    from gs_icp import IcpOptions

    o = IcpOptions()
    assert o.validated() == ((4, 4), (2, 5), (1, 10)) == R.STAGES
    assert (o.dist_max, o.cos_min, o.damping, o.alpha_min, o.edge_rel, o.normal_step, o.min_inlier_share) == \
        (0.2, 0.0, 1e-6, 0.5, 0.1, 1, 0.25)
    for bad in (dict(stages=()), dict(stages=((0, 3),)), dict(stages=((2, 0),)), dict(stages=((2, 1.5),)), dict(stages=((2,),)),
                dict(dist_max=0.0), dict(dist_max=float("nan")), dict(cos_min=float("nan")), dict(damping=-1.0),
                dict(damping=float("inf")), dict(normal_step=0), dict(min_inlier_share=1.5), dict(min_count=-1),
                dict(edge_rel=float("nan")), dict(alpha_min=float("nan"))):
        with pytest.raises(ValueError):
            IcpOptions(**bad).validated()
    assert "analytic room corner" in IcpOptions.__doc__  # the docstring says which defaults have evidence


def test_relative_pose_and_compose_round_trip():
    from gs_icp import compose, decide, relative_pose, so3_log
    from gs_track import so3_exp

    rng = np.random.default_rng(5)
    for k in range(50):
        w_m, w_f = rng.normal(size=3) * 0.8, rng.normal(size=3) * 0.8
        rot_m, rot_f = so3_exp_series(w_m), so3_exp_series(w_f)
        tran_m, tran_f = rng.normal(size=3), rng.normal(size=3)
        Rr, tr = relative_pose(rot_m, tran_m, rot_f, tran_f)
        Rq, tq = R.relative(rot_m, tran_m, rot_f, tran_f)  # the independent statement
        assert np.abs(Rr - Rq).max() < 1e-12 and np.abs(tr - tq).max() < 1e-12
        p = rng.normal(size=3)  # a world point seen by both: p_model = R p_frame + t
        assert np.abs(Rr @ (rot_f @ p + tran_f) + tr - (rot_m @ p + tran_m)).max() < 1e-12
        rot, tran = compose(rot_m, tran_m, Rr, tr)
        assert np.abs(rot - rot_f).max() < 1e-12 and np.abs(tran - tran_f).max() < 1e-12
        assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-14
        assert np.abs(so3_exp(so3_log(rot_m)) - rot_m).max() < 1e-12
    Ri, ti = relative_pose(rot_m, tran_m, rot_m, tran_m)
    assert np.abs(Ri - np.eye(3)).max() < 1e-15 and np.abs(ti).max() < 1e-15
    # the acceptance rule on hand-made logs: (kept, measured, sum e e, status) per iteration
    def log(rows):
        out = np.zeros((len(rows), 40))
        for r, (kept, meas, ee, status) in zip(out, rows):
            r[0], r[1], r[2], r[36] = kept, meas, ee, status
        return out

    assert decide(log([(100, 200, 1.0, 0), (150, 200, 0.1, 0)]), 0.25)
    assert not decide(log([(100, 200, 1.0, 0), (150, 200, 0.1, 2)]), 0.25)  # a failed solve
    assert not decide(log([(100, 200, 1.0, 1), (150, 200, 0.1, 0)]), 0.25)
    assert not decide(log([(100, 200, 1.0, 0), (49, 200, 0.01, 0)]), 0.25)   # inlier share below a quarter
    assert not decide(log([(100, 200, 1.0, 0), (100, 200, 1.5, 0)]), 0.25)   # the rmse rose
    assert not decide(log([]), 0.25)


_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "icp_point.h"
// stdin: int32 {H, W, Hm, Wm, stride, step, has_alpha}, float {fx, fy, dx, dy, fxm, fym, dxm, dym, alpha_min, edge_rel, dist_max,
// cos_min, Rt[12]}, D [Hm Wm], A [Hm Wm] (has_alpha), range [H W]
// stdout: vertex [Hm Wm 4], normal [Hm Wm 4], then per lattice pixel 30 floats (measured, kept, the 28 terms or zeros)
template <class T> static void rd(T *p, size_t n) { if (fread(p, sizeof(T), n, stdin) != n) exit(2); }
int main() {
    int32_t I[7];
    float F[24];
    rd(I, 7), rd(F, 24);
    const int H = I[0], W = I[1], Hm = I[2], Wm = I[3], stride = I[4], step = I[5];
    gs_icp_cam c{F[0], F[1], F[2], F[3], W, H, gs_icp_origin(W), gs_icp_origin(H)};
    gs_icp_cam m{F[4], F[5], F[6], F[7], Wm, Hm, gs_icp_origin(Wm), gs_icp_origin(Hm)};
    std::vector<float> D((size_t)Hm * Wm), A((size_t)Hm * Wm), z((size_t)H * W);
    rd(D.data(), D.size());
    if (I[6]) rd(A.data(), A.size());
    rd(z.data(), z.size());
    std::vector<float> V((size_t)Hm * Wm * 4), N((size_t)Hm * Wm * 4);
    const float one_plus = 1.f + F[9];
    for (int y = 0; y < Hm; ++y)
        for (int x = 0; x < Wm; ++x)
            gs_icp_model_pixel(D.data(), I[6] ? A.data() : nullptr, m, x, y, F[8], F[9], one_plus, step,
                               &V[((size_t)y * Wm + x) * 4], &N[((size_t)y * Wm + x) * 4]);
    fwrite(V.data(), 4, V.size(), stdout);
    fwrite(N.data(), 4, N.size(), stdout);
    for (int y = stride / 2; y < H; y += stride)
        for (int x = stride / 2; x < W; x += stride) {
            float out[30] = {0};
            const float r = z[(size_t)y * W + x];
            if (gs_icp_measured(r)) {
                out[0] = 1.f;
                float p[3], q[3];
                gs_icp_point(c, x, y, r, p);
                gs_icp_transform(F + 12, p, q);
                const int64_t at = gs_icp_project(m, q);
                if (at >= 0 && gs_icp_terms(q, &V[at * 4], &N[at * 4], F[10], F[11], out + 2)) out[1] = 1.f;
                else for (int k = 2; k < 30; ++k) out[k] = 0.f;
            }
            fwrite(out, 4, 30, stdout);
        }
    return 0;
}
"""


def _host_run(exe, cam, mcam, D, A, z, stride, step, alpha_min, edge_rel, dist_max, cos_min, Rm, t):
    Rt = np.concatenate([np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(np.float32)
    blob = np.array([cam.height, cam.width, mcam.height, mcam.width, stride, step, A is not None], np.int32).tobytes()
    blob += np.array([cam.focal_x, cam.focal_y, cam.dx, cam.dy, mcam.focal_x, mcam.focal_y, mcam.dx, mcam.dy, alpha_min,
                      edge_rel, dist_max, cos_min], np.float32).tobytes() + Rt.tobytes()
    blob += np.ascontiguousarray(D, np.float32).tobytes()
    if A is not None:
        blob += np.ascontiguousarray(A, np.float32).tobytes()
    blob += np.ascontiguousarray(z, np.float32).tobytes()
    out = np.frombuffer(subprocess.run([str(exe)], input=blob, stdout=subprocess.PIPE, check=True).stdout, np.float32)
    n = mcam.height * mcam.width * 4
    return out[:n].reshape(mcam.height, mcam.width, 4), out[n:2 * n].reshape(mcam.height, mcam.width, 4), out[2 * n:].reshape(-1, 30)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_point_header_compiled_for_the_host_computes_like_the_restatement(tmp_path):
    """csrc/icp_point.h is the kernels' own text; compiled for the host (no FMA contraction, IEEE division and square root) it
    gives the float32 restatement's vertices, normals, flags, keep / drop decisions and terms bit for bit: with and without
    alpha, normal_step 1 and 2, an offset principal point, differing frame and model cameras."""
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "main.cpp", tmp_path / "icp_host"
    src.write_text(_MAIN)
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    # the model maps, on the inputs of the GPU tier
    for (Hc, Wc), pp in (((7, 9), (0.0, 0.0)), ((48, 64), R.PP_OFFSET), ((37, 53), (0.0, 0.0))):
        cam, D, A, rho = R.maps_case(Hc, Wc, Hc + Wc, pp)
        z = np.ones((2, 2), np.float32)
        for step in (1, 2):
            for depth, alpha in ((D, A), (rho, None)):
                V, N, _ = _host_run(exe, R.Cam(2, 2, 1.0), cam, depth, alpha, z, 1, step, R.ALPHA_MIN, R.EDGE_REL, 0.2, 0.0,
                                    np.eye(3), np.zeros(3))
                Vr, Nr = R.model_maps(depth, alpha, cam, R.ALPHA_MIN, R.EDGE_REL, step)
                assert _same_bits(V, Vr) and _same_bits(N, Nr), (Hc, Wc, pp, step, alpha is None)
                assert 0 < Nr[..., 3].sum() < Vr[..., 3].sum() < Hc * Wc
    # one step
    cases = [R.step_case(48, 64, 11), R.step_case(37, 53, 12, model_size=(48, 64), model_pp=R.PP_OFFSET, frame_pp=(-2.5, 3.25))]
    for k in cases:
        for stride in (1, 2, 4):
            for cos_min in (0.0, 0.5):
                V, N, rows = _host_run(exe, k["cam"], k["mcam"], k["zm"], None, k["z"], stride, 1, R.ALPHA_MIN, R.EDGE_REL, 0.2,
                                       cos_min, k["R"], k["t"])
                Vr, Nr = R.model_maps(k["zm"], None, k["mcam"])
                assert _same_bits(V, Vr) and _same_bits(N, Nr)
                terms, kept, meas = R.step_terms(k["z"], k["cam"], Vr, Nr, k["mcam"], k["R"], k["t"], stride, 0.2, cos_min)
                assert int(rows[:, 0].sum()) == meas and int(rows[:, 1].sum()) == kept and kept > 0.5 * meas > 0
                assert _same_bits(rows[rows[:, 1] == 1][:, 2:], terms)


def _corner_run(rot_true, angle, shift, dtype=np.float64):
    cam = R.corner_camera()
    z = R.corner_range(rot_true, R.CORNER_TRAN).astype(np.float32)
    rot0, tran0 = perturbed_start(rot_true, R.CORNER_TRAN, angle_deg=angle, shift=shift)
    V, N = R.model_maps(R.corner_range(rot0, tran0).astype(np.float32), None, cam, dtype=dtype)
    Rr, tr, rows = R.align(z, cam, V, N, cam, np.eye(3), np.zeros(3), dtype=dtype)
    rot, tran = R.frame_pose(rot0, tran0, Rr, tr)
    return pose_errors(rot0, tran0, rot_true, R.CORNER_TRAN), pose_errors(rot, tran, rot_true, R.CORNER_TRAN), rows


def test_the_corner_is_what_the_issue_describes():
    rng, index = R.corner_range(R.CORNER_ROT, R.CORNER_TRAN, with_index=True)
    assert rng.shape == (120, 160) and (rng > 0).all()
    share = [float((index == k).mean()) for k in range(3)]
    assert [round(100 * s) for s in share] == [46, 16, 38]
    _, index = R.corner_range(R.SLIDING_ROT, R.CORNER_TRAN, with_index=True)
    assert (index == 0).sum() == 0 and (index == 1).sum() > 0 and (index == 2).sum() > 0  # the third plane is out of view


@pytest.mark.parametrize("angle,shift", R.STARTS)
def test_float64_restatement_converges_on_the_corner(angle, shift):
    """The project's tracking criterion: from 0.5 degrees / 0.02, 2 / 0.08 and 4 / 0.16 the default stages end at no more than a
    tenth of both start errors.  (The model is the corner's exact range map from the start pose.)"""
    start, end, rows = _corner_run(R.CORNER_ROT, angle, shift)
    print(f"start {start} -> end {end}; first {rows[0]}, last {rows[-1]}")
    assert len(rows) == 19 and all(r[3] == 0 for r in rows)
    assert end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1], (start, end)
    assert rows[-1][0] >= 0.25 * rows[-1][1] and rows[-1][2] <= rows[0][2]  # what `accepted` asks


@pytest.mark.parametrize("angle,shift", R.STARTS)
def test_a_corner_without_its_third_plane_slides(angle, shift):
    """With the plane x = -1.2 out of view nothing holds the camera along the remaining edge: the rotation converges, the
    residual falls as far as on the full corner, and the translation does NOT converge -- it ends further off than it started.
    The residual cannot tell: this is why IcpResult carries its counts and log, and why `accepted` is only a necessary test."""
    start, end, rows = _corner_run(R.SLIDING_ROT, angle, shift)
    _, _, full = _corner_run(R.CORNER_ROT, angle, shift)
    print(f"start {start} -> end {end}; first {rows[0]}, last {rows[-1]}")
    assert end[0] <= 0.1 * start[0]
    assert end[1] > start[1] and end[1] > 0.1                  # the slide
    assert rows[-1][2] <= 0.1 * rows[0][2] and rows[-1][2] <= 2.0 * full[-1][2]   # ... under a converged residual
    assert rows[-1][0] >= 0.25 * rows[-1][1] and all(r[3] == 0 for r in rows)  # `accepted` would hold


def test_slam_options_and_frame_keep_their_prefix():
    import gs_slam
    from gs_icp import IcpOptions, IcpResult

    assert gs_slam.SlamOptions().icp is None
    assert list(gs_slam.SlamOptions.__dataclass_fields__)[-1] == "icp"
    fields = list(gs_slam.SlamFrame.__dataclass_fields__)
    assert fields[:8] == ["rot", "tran", "tracked", "keyframe", "overlap", "window", "added", "map_losses"]
    assert fields[-1] == "icp" and gs_slam.SlamFrame.__dataclass_fields__["icp"].default is None
    assert gs_slam.IcpOptions is IcpOptions and gs_slam.IcpResult is IcpResult
    with pytest.raises(ValueError):  # a bad schedule is refused when the loop is built, before any device work
        IcpOptions(stages=((0, 1),)).validated()
