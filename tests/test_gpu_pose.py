"""GPU tier of the camera pose gradients (GS_FRAME_POSE_GRAD, include/gs_abi.h; FrameRenderer.backward(grad_pose=...) and
render / render_aux(..., pose=(rot, tran))).

Yardsticks:
  1. the fp64 oracle: OracleFrame.backward_f64's rows (plus, for aux frames, the depth / alpha rows of the oracle with the maps
     posed as colours, tests/test_gpu_aux.py), summed per Gaussian and pushed through oracle/torch_ref.project (J detached)
     with rot / tran requiring grad; the fp32 oracle's rows through the same projection give the reference's own error;
  2. identities that hold exactly in exact arithmetic between the pose gradient and the per-Gaussian gradients of the SAME
     backward: a camera translation, a camera rotation and a uniform scaling of rot are the same as moving / rotating /
     scaling every Gaussian the other way (the J-detached convention makes this exact);
  3. the per-Gaussian gradients and images of flagged frames are bit-identical to those of unflagged ones;
  4. repeatability, the backward in parts, zeros for an empty frame;
  5. autograd against the low-level call; 6. a pose fit that converges.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera
from gs_testutil import OracleFrame, _sum_by_id, to_torch
from test_gpu_aux import _random_grads, aux_colours, case

pytestmark = pytest.mark.gpu


def _f64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _pose_through_projection(of, d_pos_i, d_cov):
    """dL/drot, dL/dtran in double: per-Gaussian dL/dpos_i, dL/dcov2d through oracle/torch_ref.project (J detached)."""
    from oracle import torch_ref

    vis = np.nonzero(of.mask)[0]
    rot = _f64(of.cam.rot).requires_grad_(True)
    tran = _f64(of.cam.tran).requires_grad_(True)
    pos_i, cov = torch_ref.project(_f64(of.scene.pos[vis]), _f64(of.qn[vis]), _f64(of.sn[vis]), rot, tran,
                                   detach_jacobian=True)
    obj = (pos_i * _f64(d_pos_i[vis])).sum() + (cov.reshape(-1, 4) * _f64(d_cov[vis])).sum()
    g_rot, g_tran = torch.autograd.grad(obj, (rot, tran))
    return np.concatenate([g_rot.numpy().reshape(9), g_tran.numpy()])


def _pose_scale(of, d_pos_i, d_cov):
    """S_c = sum_i |term_i,c| in double: the same projection restated with a copy of rot / tran per Gaussian."""
    vis = np.nonzero(of.mask)[0]
    n = len(vis)
    R = _f64(of.cam.rot).expand(n, 3, 3).clone().requires_grad_(True)
    T = _f64(of.cam.tran).expand(n, 3).clone().requires_grad_(True)
    p, q, s = _f64(of.scene.pos[vis]), _f64(of.qn[vis]), _f64(of.sn[vis])
    pc = torch.einsum("nij,nj->ni", R, p) + T
    x, y, z = pc.unbind(-1)
    pos_i = torch.stack([x / z, y / z, pc.norm(dim=-1)], -1)
    zero = torch.zeros_like(z)
    J = torch.stack([1 / z, zero, -x / (z * z), zero, 1 / z, -y / (z * z)], -1).reshape(-1, 2, 3).detach()
    w, a, b, c = q.unbind(-1)
    Rg = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w),
                      2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w),
                      2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1).reshape(-1, 3, 3)
    M = Rg * s.unsqueeze(-2)
    JW = J @ R
    cov = JW @ (M @ M.transpose(-1, -2)) @ JW.transpose(-1, -2)
    obj = (pos_i * _f64(d_pos_i[vis])).sum() + (cov.reshape(-1, 4) * _f64(d_cov[vis])).sum()
    gR, gT = torch.autograd.grad(obj, (R, T))
    terms = torch.cat([gR.reshape(n, 9), gT], 1).numpy()
    return terms.sum(0), np.abs(terms).sum(0)


def _aux_rows(of, gd, ga, f64):
    """(d_pos_i, d_cov) contributions of the depth / alpha maps' gradients (the oracle with the maps posed as colours)."""
    g = of.grid
    top, left = g.crop_offsets()
    cols = aux_colours(of)
    out = oracle.draw(of.s_pos, cols, of.s_opa, of.s_cov, of.accum, g.padded_height, g.padded_width, g.focal_x, g.focal_y,
                      use_sh=False, fast=True)
    gpad = np.zeros_like(out)
    gpad[top:top + g.height, left:left + g.width, 0] = gd
    gpad[top:top + g.height, left:left + g.width, 1] = ga
    if f64:
        gp, gr, _, gc = oracle.draw_backward_f64(of.s_pos, cols, of.s_opa, of.s_cov, of.accum, gpad, g.focal_x, g.focal_y,
                                                 use_sh=False)
    else:
        gp, gr, _, gc = oracle.draw_backward(of.s_pos, cols, of.s_opa, of.s_cov, of.accum, out, gpad, g.focal_x, g.focal_y,
                                             use_sh=False, fast=True)
    n = of.scene.n
    d_pos_i, d_cov = _sum_by_id(of.ids, gp, n), _sum_by_id(of.ids, gc, n)
    d_pos_i[:, 2] += _sum_by_id(of.ids, gr[:, 0], n)
    return d_pos_i, d_cov


def _pose_buffers(gpu, fill=float("nan")):
    return (torch.full((3, 3), fill, device=gpu, dtype=torch.float32), torch.full((3,), fill, device=gpu, dtype=torch.float32))


def _flat(gp):
    return torch.cat([gp[0].reshape(9), gp[1]]).double().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("aux", [False, True])
def test_pose_gradient_matches_fp64_oracle(gpu, aux):
    check_pose_gradient(gpu, *case(5000, 128, 96, seed=31), aux)


def check_pose_gradient(gpu, scene, cam, aux, of=None):
    """-> worst err / tol over the twelve components"""
    of = OracleFrame(scene, cam) if of is None else of
    gimg, gd, ga = _random_grads(of, 37)
    n = scene.n
    # truth: the fp64 rows; the reference's own error: the fp32 oracle's rows, both through the same fp64 projection
    rows64, _ = of.backward_f64(gimg)
    d_pos64, d_cov64 = _sum_by_id(of.ids, rows64[0], n), _sum_by_id(of.ids, rows64[3], n)
    of.backward(gimg)
    d_pos32, d_cov32 = _sum_by_id(of.ids, of.pair_grads[0], n), _sum_by_id(of.ids, of.pair_grads[3], n)
    if aux:
        a64, a32 = _aux_rows(of, gd, ga, True), _aux_rows(of, gd, ga, False)
        d_pos64, d_cov64 = d_pos64 + a64[0], d_cov64 + a64[1]
        d_pos32, d_cov32 = d_pos32 + a32[0], d_cov32 + a32[1]
    truth = _pose_through_projection(of, d_pos64, d_cov64)
    ref32 = _pose_through_projection(of, d_pos32, d_cov32)
    total, S = _pose_scale(of, d_pos64, d_cov64)
    assert np.allclose(total, truth, rtol=1e-9, atol=1e-12 * S.max())  # (the restatement agrees with torch_ref)

    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    params = to_torch(scene, gpu)
    r.forward(*params, cam, aux=aux)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    gp = _pose_buffers(gpu)
    if aux:
        r.backward(t(gimg), grad_depth=t(gd), grad_alpha=t(ga), grad_pose=gp)
    else:
        r.backward(t(gimg), grad_pose=gp)
    got = _flat(gp)
    tol = 4 * np.maximum(np.abs(ref32 - truth), 1e-6 * S)
    err = np.abs(got - truth)
    assert np.all(err <= tol), (got, truth, err / np.maximum(S, 1e-30), tol / np.maximum(S, 1e-30))
    assert np.abs(truth).max() > 1e-3 * S.max()  # (a gradient that says something)
    return float((err / tol).max())


# ------------------------------------------------------------------------------------------------------------ 2. identities
def _skew(k):
    e = np.eye(3)[k]
    return torch.from_numpy(np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]]))


def _check_identities(rot, params, grads, gp, scale_act_abs=True):
    """The pose gradient against the same backward's per-Gaussian gradients (all in double on the device)."""
    dev = params[0].device
    R = torch.as_tensor(np.asarray(rot, np.float64), device=dev)
    Gr = gp[0].double()
    Gt = gp[1].double()
    p = params[0].double()
    q = params[1].double()
    s = params[2].double()
    g_pos, g_quat, g_scale = (g.double() for g in grads[:3])
    # translation: dL/dtran = rot . sum_i grad_pos_i   (grad_pos = rot^T gc)
    terms = g_pos @ R.T
    lhs, rhs, mag = Gt, terms.sum(0), terms.abs().sum(0)
    assert torch.all((lhs - rhs).abs() <= 1e-5 * mag + 1e-30), (lhs, rhs, mag)
    # rotation, right perturbation rot -> rot exp([w]x): every Gaussian rotated by exp([w]x)
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64, device=dev)
        e[k] = 1.0
        lhs = torch.trace(Gr.T @ R @ _skew(k).to(dev))
        t_pos = (torch.cross(p, g_pos, dim=1) * e).sum(1)  # e_k . (p_i x grad_pos_i)
        # 1/2 (0, e_k) (x) q_i  (quaternion product, (w, x, y, z))
        qw, qv = q[:, 0], q[:, 1:]
        dq = torch.cat([(-(qv * e).sum(1))[:, None], qw[:, None] * e + torch.cross(e.expand_as(qv), qv, dim=1)], 1) * 0.5
        t_quat = (g_quat * dq).sum(1)
        rhs = t_pos.sum() + t_quat.sum()
        mag = t_pos.abs().sum() + t_quat.abs().sum()
        assert abs(float(lhs - rhs)) <= 1e-5 * float(mag), (k, float(lhs), float(rhs), float(mag))
    # uniform scaling of rot (scale_activation "abs": the activated scale is |s| + 1e-4)
    if scale_act_abs:
        lhs = torch.trace(Gr.T @ R)
        t_pos = (p * g_pos).sum(1)
        t_s = (g_scale * (s.abs() + 1e-4) * torch.sign(s)).sum(1)
        rhs, mag = t_pos.sum() + t_s.sum(), t_pos.abs().sum() + t_s.abs().sum()
        assert abs(float(lhs - rhs)) <= 1e-5 * float(mag), (float(lhs), float(rhs), float(mag))


def _identity_case(gpu, scene, cam, aux, bwd_rows, seed):
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=True, bwd_rows=bwd_rows)
    image, *_ = r.forward(*params, cam, aux=aux)
    assert not r.stats().overflow
    g = torch.Generator(device=gpu).manual_seed(seed)
    gimg = torch.randn(image.shape, generator=g, device=gpu)
    kw = {}
    if aux:
        kw = dict(grad_depth=torch.randn(image.shape[:2], generator=g, device=gpu),
                  grad_alpha=torch.randn(image.shape[:2], generator=g, device=gpu))
    gp = _pose_buffers(gpu)
    grads = r.backward(gimg, grad_pose=gp, **kw)
    assert torch.isfinite(gp[0]).all() and torch.isfinite(gp[1]).all()
    _check_identities(cam.rot, params, grads, gp)
    return r


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("bwd_rows", [False, True])
def test_pose_identities_small(gpu, aux, bwd_rows):
    scene, cam = case(5000, 128, 96, seed=41)
    _identity_case(gpu, scene, cam, aux, bwd_rows, 43)


@pytest.mark.parametrize("aux", [False, True])
def test_pose_identities_with_workgroup_summed_gaussians(gpu, aux):
    """Gaussians covering more than GS_PB_BIG = 64 tiles are summed by the whole workgroup before the epilogue."""
    scene, cam = case(8000, 192, 128, seed=47, max_px_sigma=48.0)
    r = _identity_case(gpu, scene, cam, aux, False, 53)
    assert int((r._rects()[:, 3] > 64).sum()) > 0


_FULL = {}


@pytest.mark.parametrize("n", [376_467, 2_400_000])
@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("bwd_rows", [False, True])
def test_pose_identities_full_size(gpu, n, aux, bwd_rows):
    """Thousands of partial rows (9,376 workgroups of the projection backward at 2.4 M Gaussians)."""
    if n not in _FULL:
        _FULL.clear()
        _FULL[n] = case(n, 1920, 1080, seed=59)
    scene, cam = _FULL[n]
    _identity_case(gpu, scene, cam, aux, bwd_rows, 61)


# ------------------------------------------------------------------------------------------------------ 3. nothing else moves
@pytest.mark.parametrize("aux", [False, True])
def test_flagged_backward_leaves_the_gaussian_gradients_alone(gpu, aux):
    scene, cam = case(20_000, 160, 112, seed=67)
    of = OracleFrame(scene, cam)
    gimg, gd, ga = _random_grads(of, 71)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    kw = dict(grad_depth=t(gd), grad_alpha=t(ga)) if aux else {}
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    params = to_torch(scene, gpu)
    r.forward(*params, cam, aux=aux)
    plain = [x.clone() for x in r.backward(t(gimg), **kw)]
    flagged = r.backward(t(gimg), grad_pose=_pose_buffers(gpu), **kw)
    for a, b in zip(plain, flagged):
        assert torch.equal(a, b)
    assert not (r._frame.flags & _lib.GS_FRAME_POSE_GRAD)  # (the renderer's own descriptor stays unflagged)


def test_render_with_pose_equals_render_with_posed_camera(gpu):
    scene, cam = case(5000, 128, 96, seed=73)
    params = to_torch(scene, gpu)
    rot = torch.from_numpy(cam.rot.copy())
    tran = torch.from_numpy(cam.tran.copy())
    base = make_camera(128, 96)  # identity pose: the pose tensors carry case()'s
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    a = r.render(*params, cam)
    b = r.render(*params, base, pose=(rot, tran))
    c = r.render(*params, base, pose=(rot.to(gpu), tran.to(gpu)))
    assert torch.equal(a, b) and torch.equal(a, c)
    ai, ad, aa = r.render_aux(*params, cam)
    bi, bd, ba = r.render_aux(*params, base, pose=(rot, tran))
    assert torch.equal(ai, bi) and torch.equal(ad, bd) and torch.equal(aa, ba)


# ---------------------------------------------------------------------------------------------- 4. repeatable, parts, empty
@pytest.mark.parametrize("aux", [False, True])
def test_pose_gradient_repeatable_and_in_parts(gpu, aux):
    scene, cam = case(20_000, 160, 112, seed=79)
    of = OracleFrame(scene, cam)
    gimg, gd, ga = _random_grads(of, 83)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    kw = dict(grad_depth=t(gd), grad_alpha=t(ga)) if aux else {}
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    params = to_torch(scene, gpu)
    r.forward(*params, cam, aux=aux)
    gp1, gp2, gp3 = _pose_buffers(gpu), _pose_buffers(gpu), _pose_buffers(gpu)
    full = [x.clone() for x in r.backward(t(gimg), grad_pose=gp1, **kw)]
    r.backward(t(gimg), grad_pose=gp2, **kw)
    assert torch.equal(gp1[0], gp2[0]) and torch.equal(gp1[1], gp2[1])
    out = tuple(torch.full_like(x, float("nan")) for x in full)
    r.backward(t(gimg), out=out, part=_lib.GS_BWD_RASTER, **kw)
    r.backward(None, out=out, part=_lib.GS_BWD_GEOMETRY, grad_pose=gp3)
    r.backward(None, out=out, part=_lib.GS_BWD_COLOR)
    assert torch.equal(gp1[0], gp3[0]) and torch.equal(gp1[1], gp3[1])
    for a, b in zip(full, out):
        assert torch.equal(a, b)
    # GS_BWD_COLOR (and GS_BWD_RASTER) of a flagged frame leave the pose buffers alone (the C ABI: the Python wrapper only
    # takes grad_pose where it is written)
    nan = _pose_buffers(gpu)
    f = r._pose_frame(r._frame, nan, 0)
    with torch.cuda.device(gpu):
        _lib.check(_lib.gs_frame_backward_part(ctypes.byref(f), None, *(x.data_ptr() for x in out), _lib.GS_BWD_COLOR,
                                               torch.cuda.current_stream(gpu).cuda_stream), "gs_frame_backward_part")
    torch.cuda.synchronize(gpu)
    assert torch.isnan(nan[0]).all() and torch.isnan(nan[1]).all()
    for a, b in zip(full, out):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError):
        r.backward(None, out=out, part=_lib.GS_BWD_COLOR, grad_pose=_pose_buffers(gpu))


def test_empty_frame_writes_zeros(gpu):
    """N = 0: no kernel runs, the pose gradient is written (zeros) all the same -- never left stale."""
    cam = make_camera(128, 96)
    z = lambda *s: torch.zeros(*s, device=gpu, dtype=torch.float32)  # noqa: E731
    params = (z(0, 3), z(0, 4), z(0, 3), z(0), z(0, 3))
    dummy = z(64)  # (the gradient destinations of N = 0 Gaussians: never written, but not NULL)
    r = FrameRenderer(gpu, max_pairs=1 << 12, training=True, auto_grow=False)
    stream = lambda: torch.cuda.current_stream(gpu).cuda_stream  # noqa: E731
    for aux in (False, True):
        image, *_ = r.forward(*params, cam, aux=aux)
        gimg = torch.ones_like(image)
        gp = _pose_buffers(gpu)
        f = r._pose_frame(r._frame, gp, 0)
        with torch.cuda.device(gpu):
            _lib.check(_lib.gs_frame_backward(ctypes.byref(f), gimg.data_ptr(), *([dummy.data_ptr()] * 5), stream()),
                       "gs_frame_backward")
        assert torch.equal(gp[0], z(3, 3)) and torch.equal(gp[1], z(3))
        gp = _pose_buffers(gpu)
        f = r._pose_frame(r._frame, gp, _lib.GS_BWD_GEOMETRY)
        with torch.cuda.device(gpu):
            _lib.check(_lib.gs_frame_backward_part(ctypes.byref(f), None, *([dummy.data_ptr()] * 5), _lib.GS_BWD_GEOMETRY,
                                                   stream()), "gs_frame_backward_part")
        assert torch.equal(gp[0], z(3, 3)) and torch.equal(gp[1], z(3))


# ---------------------------------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("pose_device", ["cpu", "gpu"])
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("aux", [False, True])
def test_autograd_pose_gradients_equal_the_low_level_call(gpu, pose_device, frozen, aux):
    scene, cam = case(5000, 128, 96, seed=89)
    dev = gpu if pose_device == "gpu" else torch.device("cpu")
    rot = torch.from_numpy(cam.rot.copy()).to(dev).requires_grad_(True)
    tran = torch.from_numpy(cam.tran.copy()).to(dev).requires_grad_(True)
    params = to_torch(scene, gpu, requires_grad=not frozen)
    base = make_camera(128, 96)
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    g = torch.Generator(device=gpu).manual_seed(97)
    w = torch.randn(96, 128, 3, generator=g, device=gpu)
    wd, wa = torch.randn(96, 128, generator=g, device=gpu), torch.randn(96, 128, generator=g, device=gpu)
    if aux:
        image, depth, alpha = r.render_aux(*params, base, pose=(rot, tran))
        ((image * w).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
    else:
        (r.render(*params, base, pose=(rot, tran)) * w).sum().backward()
    assert rot.grad is not None and tran.grad is not None and rot.grad.device == dev and tran.grad.device == dev
    assert all(p.grad is None for p in params) if frozen else all(p.grad is not None for p in params)
    # the low-level call on the same frame
    r2 = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    p2 = to_torch(scene, gpu)
    r2.forward(*p2, cam, aux=aux)
    gp = _pose_buffers(gpu)
    ref = r2.backward(w, grad_pose=gp, **(dict(grad_depth=wd, grad_alpha=wa) if aux else {}))
    assert torch.equal(rot.grad.to(gpu), gp[0]) and torch.equal(tran.grad.to(gpu), gp[1])
    if not frozen:
        for a, b in zip(params, ref):
            assert torch.equal(a.grad, b)


def test_pose_gradient_refused_for_sh_scenes(gpu):
    scene, cam = case(3000, 128, 96, seed=101, use_sh=True)
    params = to_torch(scene, gpu)
    rot = torch.from_numpy(cam.rot.copy()).requires_grad_(True)
    tran = torch.from_numpy(cam.tran.copy())
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    with pytest.raises(RuntimeError, match="rgb colours"):
        r.render(*params, cam, pose=(rot, tran))
    with pytest.raises(RuntimeError, match="rgb colours"):
        r.render_aux(*params, cam, pose=(rot, tran))
    # a pose that needs no gradient is only a camera
    img = r.render(*params, make_camera(128, 96), pose=(rot.detach(), tran))
    assert torch.equal(img, r.render(*params, cam))


# ------------------------------------------------------------------------------------------------------------ 6. pose fit
def _axis_angle(w):
    K = torch.zeros(3, 3, dtype=w.dtype)
    K[0, 1], K[0, 2], K[1, 2] = -w[2], w[1], -w[0]
    K[1, 0], K[2, 0], K[2, 1] = w[2], -w[1], w[0]
    return torch.linalg.matrix_exp(K)


@pytest.mark.parametrize("with_depth", [False, True])
def test_pose_recovery(gpu, with_depth):
    W, H = 160, 120
    scene, cam = case(20_000, W, H, seed=103)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 19, training=True, auto_grow=True)
    R_true = torch.from_numpy(cam.rot.astype(np.float64))
    t_true = torch.from_numpy(cam.tran.astype(np.float64))
    with torch.no_grad():
        tgt_img, tgt_d, tgt_a = r.render_aux(*params, cam)
        tgt_ed = tgt_d / tgt_a.clamp_min(1e-3)
    rng = np.random.default_rng(107)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R0 = _axis_angle(torch.from_numpy(axis * math.radians(0.5))) @ R_true
    sh = rng.normal(size=3)
    t0 = t_true + torch.from_numpy(sh / np.linalg.norm(sh) * 0.02)
    w = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    t = t0.clone().requires_grad_(True)
    opt = torch.optim.Adam([w, t], lr=2e-3)
    iters = 300
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.01 ** (k / iters))

    def errors():
        with torch.no_grad():
            Rk = _axis_angle(w) @ R0
            return float(torch.linalg.norm(Rk - R_true) / math.sqrt(2.0)), float(torch.linalg.norm(t - t_true))

    e_r0, e_t0 = errors()
    for _ in range(iters):
        opt.zero_grad()
        rot = (_axis_angle(w) @ R0).float()
        tran = t.float()
        if with_depth:
            img, d, a = r.render_aux(*params, cam, pose=(rot, tran))
            ed = d / a.clamp_min(1e-3)
            mask = (tgt_a > 0.5) & (a.detach() > 0.5)
            loss = (img - tgt_img).abs().mean() + ((ed - tgt_ed).abs() * mask).mean()
        else:
            loss = (r.render(*params, cam, pose=(rot, tran)) - tgt_img).abs().mean()
        loss.backward()
        opt.step()
        sched.step()
    e_r, e_t = errors()
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
