"""GPU tier of RGB-D training: the depth loss kernel (gs_loss_depth) against an fp64 evaluation of its formulas, the fused
backward + Adam step of aux frames (gs_frame_backward_adam_aux) bit for bit against gs_frame_backward + gs_adam_step, the
Trainer's depth-supervised step, and a fit in which depth supervision has to help.  include/gs_abi.h states the contracts."""
import math

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_dp import FlatGaussianParams
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import depth_loss_f64, to_torch
from gs_train import DepthLoss, FusedAdam, TrainOptions, Trainer, base_lrs, z_to_range

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- 1. the loss kernel
def _loss_inputs(H, W, mode, alpha_min, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.02, 1.0, (H, W)).astype(np.float32)  # mode 1: straddles alpha_min = 0.5
    z = rng.uniform(0.3, 12.0, (H, W)).astype(np.float32)
    D = (A * z * rng.uniform(0.7, 1.3, (H, W))).astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.30  # 30 % of the target carries no measurement: 0, negative, inf, NaN
    kind = rng.integers(0, 4, (H, W))
    z[bad & (kind == 0)] = 0.0
    z[bad & (kind == 1)] = -z[bad & (kind == 1)]
    z[bad & (kind == 2)] = np.inf
    z[bad & (kind == 3)] = np.nan
    return D, A, z


@pytest.mark.parametrize("mode", ["residual", "expected"])
@pytest.mark.parametrize("H,W", [(48, 64), (187, 250), (1080, 1920)])
def test_depth_loss_matches_fp64(gpu, H, W, mode):
    """gs_loss_depth against torch in fp64.  Gradients within 1e-6 |ref| (at most ~10 fp32 roundings of 2^-24 each); pixels
    whose fp64 |r| is below 1e-6 max(|D|, |A z|) are left out (the sign is not decidable in fp32), at most 0.1 % of them;
    gradients exactly zero where the pixel does not count; the loss within 1e-5 relative, the count exact; two runs bitwise
    equal."""
    alpha_min, scale = 0.5, 0.37 / (H * W)
    D, A, z = _loss_inputs(H, W, mode, alpha_min, seed=H + W)
    dl = DepthLoss(H, W, mode, alpha_min, gpu)
    tD, tA, tz = (torch.from_numpy(x).to(gpu) for x in (D, A, z))
    gd, ga = dl(tD, tA, tz, scale)
    gd, ga, vals = gd.clone(), ga.clone(), dl.values.clone()
    dl.grad_depth.fill_(7.0)
    dl.grad_alpha.fill_(7.0)
    gd2, ga2 = dl(tD, tA, tz, scale)
    assert torch.equal(gd, gd2) and torch.equal(ga, ga2) and torch.equal(vals, dl.values)  # bitwise repeatable
    # fp64 reference (gs_testutil.depth_loss_f64: the one statement of the loss the aux gradient tests use too)
    ref_gd, ref_ga, ref_loss, ref_n, r, valid = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x
                                                 for x in depth_loss_f64(D, A, z, mode, alpha_min, scale))
    D64, A64, z64 = (torch.from_numpy(x.astype(np.float64)) for x in (D, A, z))
    zz = torch.where(valid, z64, torch.ones_like(z64))
    undecidable = valid & (r.abs() < 1e-6 * torch.maximum(D64.abs(), (A64 * zz).abs()))
    share = float(undecidable.sum()) / (H * W)
    got_gd, got_ga = gd.cpu().double(), ga.cpu().double()
    check = valid & ~undecidable
    e_gd = float(((got_gd - ref_gd).abs() / ref_gd.abs().clamp_min(1e-300))[check].max())
    e_ga = float(((got_ga - ref_ga).abs() / ref_ga.abs().clamp_min(1e-300))[check].max())
    v = vals.cpu().numpy()
    print(f"depth loss {mode} {W}x{H}: rel err grad_depth {e_gd:.2e} grad_alpha {e_ga:.2e}, undecidable share {share:.2e}, "
          f"loss {v[0]:.6f} vs {ref_loss:.6f}, counted {int(v[1])} vs {ref_n}")
    assert share <= 1e-3
    assert e_gd <= 1e-6 and e_ga <= 1e-6
    assert float(got_gd[~valid].abs().max()) == 0.0 and float(got_ga[~valid].abs().max()) == 0.0
    assert abs(float(v[0]) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert int(v[1]) == ref_n
    assert 0.2 * H * W < ref_n < 0.8 * H * W


# ---------------------------------------------------------------------------------- 2. fused = unfused, bit for bit
def _fused_pair(gpu, scene, cam, stat, with_image, steps, max_pairs, seed=5, probe=None, aux=True):
    """`steps` optimizer steps from identical copies through backward_adam(aux) and through backward + FusedAdam.step, random
    dL/dimage (or None), dL/ddepth, dL/dalpha per step.  Returns the two end states.  ``aux=False``: plain frames, dL/dimage
    alone, through gs_frame_backward_adam."""
    H, W = cam.height, cam.width
    start = to_torch(scene, gpu)
    lrs = [b * 0.5 for b in base_lrs(TrainOptions())]
    out = []
    for fuse in (True, False):
        gen = torch.Generator(gpu).manual_seed(seed)
        flat = FlatGaussianParams([t.clone() for t in start])
        opt = FusedAdam(flat, lrs, grad_stat=stat)
        r = FrameRenderer(gpu, max_pairs=max_pairs, training=True, auto_grow=True)
        for _ in range(steps):
            r.forward(*flat.params, cam, aux=aux)
            assert not r.last_frame_overflowed(wait=True)
            if probe is not None:
                probe(r)
            gimg = torch.randn(H, W, 3, device=gpu, generator=gen) if with_image else None
            gdep = torch.randn(H, W, device=gpu, generator=gen) * 0.1
            galp = torch.randn(H, W, device=gpu, generator=gen)
            maps = dict(grad_depth=gdep, grad_alpha=galp) if aux else {}
            opt.skip_flag = r.overflow_flag()
            if fuse:
                r.backward_adam(gimg, opt.fused_descriptor(), **maps)
            else:
                r.backward(gimg, out=flat.grads, **maps)
                opt.step()
        assert opt.step_count == steps
        out.append((flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(),
                    opt.accum_grad.clone() if opt.accum_grad is not None else torch.zeros(1, device=gpu)))
        del r, opt, flat
        torch.cuda.empty_cache()
    return out


def _assert_same(got, stat):
    for a, b, name in zip(got[0], got[1], ("parameters", "exp_avg", "exp_avg_sq", "grad statistic")):
        assert torch.equal(a, b), name
    assert float(got[0][1].abs().max()) > 0
    if stat is not None:
        assert float(got[0][3].abs().max()) > 0


@pytest.mark.parametrize("n,W,H,stat,sh,with_image", [
    (6_000, 160, 112, "max", 0, True), (6_000, 160, 112, "mean", 0, False), (6_001, 160, 112, None, 0, True),
    (6_000, 160, 112, "max", 2, True), (6_001, 160, 112, "mean", 3, False), (6_000, 160, 112, None, 3, True),
    (6_001, 160, 112, None, 2, False),
    (2_400_000, 1920, 1080, "max", 0, True), (724_312, 1920, 1080, "max", 2, True)])
def test_fused_aux_step_equals_backward_then_adam(gpu, n, W, H, stat, sh, with_image):
    """gs_frame_backward_adam_aux against gs_frame_backward (aux) + gs_adam_step: parameters, both moments and the |dL/dpos|
    statistic BIT FOR BIT over several steps -- rgb, SH degree 2 and 3; stat_mode 0 / 1 / 2; the scene sizes of
    test_gpu_train.py::test_fused_backward_adam_equals_backward_then_adam (6,001: the float4 walk's ragged end; 2.4 M rgb and
    724,312 x SH2: the non-temporal variant); random dL/dimage, dL/ddepth, dL/dalpha, and dL/dimage = None."""
    scene = make_scene(n, W, H, seed=11, use_sh=bool(sh), sh_degree=sh) if sh else make_scene(n, W, H, seed=11)
    cam = make_camera(W, H, yaw_deg=3.0)
    steps = 2 if n > 100_000 else 4
    got = _fused_pair(gpu, scene, cam, stat, with_image, steps, max_pairs=1 << 20)
    _assert_same(got, stat)


@pytest.mark.parametrize("sh", [2, 3])
def test_fused_aux_step_on_the_sh_big_rows_path(gpu, sh):
    """Gaussians of more than GS_PB_SH_BIG = 64 tiles: sh_big_rows_kernel has left the total of their rows -- the depth float
    included -- in the first row, and both paths must take g_d from there."""
    W, H = 250, 186
    scene = make_scene(1_500, W, H, seed=29, use_sh=True, sh_degree=sh, max_px_sigma=60.0)
    cam = make_camera(W, H, yaw_deg=2.0)
    seen = []

    def probe(r):
        rc = r._rects()
        seen.append(int(((rc[:, 2] != 0) & (rc[:, 3] > 64)).sum()))

    got = _fused_pair(gpu, scene, cam, "max", True, 3, max_pairs=1 << 20, probe=probe)
    assert min(seen) > 0, seen  # the path is reached in every frame
    _assert_same(got, "max")


# ------------------------------------------------------------------- 3. overflow, outputs, the plain frame's fused step
@pytest.mark.parametrize("use_sh", [False, True])
def test_fused_aux_step_skips_overflowed_frames(gpu, use_sh):
    W, H = 128, 96
    cam = make_camera(W, H)
    p = [t.clone() for t in to_torch(make_scene(4000, W, H, seed=4, use_sh=use_sh), gpu)]
    flat = FlatGaussianParams(p)
    opt = FusedAdam(flat, base_lrs(TrainOptions()), grad_stat="max")
    r = FrameRenderer(gpu, max_pairs=64, training=True, auto_grow=False)  # far too small: the frame overflows
    r.forward(*flat.params, cam, aux=True)
    assert r.stats().overflow > 0
    before = flat.flat_param.clone()
    opt.skip_flag = r.overflow_flag()
    opt.exp_avg.fill_(0.5)  # momentum that WOULD move the parameters
    r.backward_adam(torch.ones(H, W, 3, device=gpu), opt.fused_descriptor(), grad_depth=torch.ones(H, W, device=gpu),
                    grad_alpha=torch.ones(H, W, device=gpu))
    torch.cuda.synchronize()
    assert torch.equal(flat.flat_param, before)
    assert float((opt.exp_avg - 0.5).abs().max()) == 0.0 and float(opt.exp_avg_sq.abs().max()) == 0.0


def test_aux_outputs_are_untouched_and_plain_frames_step_as_before(gpu):
    W, H = 160, 112
    scene, cam = make_scene(6_000, W, H, seed=11), make_camera(W, H, yaw_deg=3.0)
    start = to_torch(scene, gpu)
    lrs = base_lrs(TrainOptions())
    # the image and the maps of an aux frame: what a renderer that never takes the new path renders, before and after it
    ref = FrameRenderer(gpu, max_pairs=1 << 20, training=True)
    want = [t.clone() for t in ref.forward(*[t.clone() for t in start], cam, aux=True)]
    flat = FlatGaussianParams([t.clone() for t in start])
    opt = FusedAdam(flat, lrs, grad_stat="max")
    r = FrameRenderer(gpu, max_pairs=1 << 20, training=True)
    outs = r.forward(*flat.params, cam, aux=True)
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    g = torch.Generator(gpu).manual_seed(1)
    gimg, gdep, galp = (torch.randn(H, W, 3, device=gpu, generator=g), torch.randn(H, W, device=gpu, generator=g),
                        torch.randn(H, W, device=gpu, generator=g))
    r.backward_adam(gimg, opt.fused_descriptor(), grad_depth=gdep, grad_alpha=galp)
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    assert not torch.equal(flat.params[0], start[0])
    # the shape / dtype checks of backward()
    r.forward(*flat.params, cam, aux=True)
    with pytest.raises(RuntimeError):
        r.backward_adam(gimg, opt.fused_descriptor(advance=False), grad_depth=gdep[:-1])
    with pytest.raises(RuntimeError):
        r.backward_adam(gimg, opt.fused_descriptor(advance=False), grad_alpha=galp.double())
    with pytest.raises(RuntimeError):
        r.backward_adam(gimg[:, :-1], opt.fused_descriptor(advance=False))
    # a plain frame: backward_adam is what it was (= backward + step, unchanged code), and refuses the new arguments
    ends = []
    for fuse in (True, False):
        flat = FlatGaussianParams([t.clone() for t in start])
        opt = FusedAdam(flat, lrs, grad_stat="max")
        r = FrameRenderer(gpu, max_pairs=1 << 20, training=True)
        for _ in range(3):
            r.forward(*flat.params, cam)
            if fuse:
                with pytest.raises(RuntimeError):
                    r.backward_adam(gimg, opt.fused_descriptor(advance=False), grad_depth=gdep)
                r.backward_adam(gimg, opt.fused_descriptor())
            else:
                r.backward(gimg, out=flat.grads)
                opt.step()
        ends.append((flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.accum_grad.clone()))
    for a, b in zip(*ends):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- 4. Trainer
def _truth(gpu, scene, cams):
    """Truth images and truth range maps (depth / alpha where alpha >= 0.5, else 0 = no measurement) of `cams`."""
    gt = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 20, auto_grow=True)
    images, ranges = [], []
    for cam in cams:
        img, _, d, a = r.forward(*gt, cam, training=False, aux=True)
        images.append(img.clone())
        ranges.append(torch.where(a >= 0.5, d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous())
    return images, ranges


def _cams(W, H, shifts):
    out = []
    for yaw, tx in shifts:
        c = make_camera(W, H, yaw_deg=yaw)
        c.tran = np.array([tx, 0.0, 0.0], np.float32)
        out.append(c)
    return out


def test_trainer_depth_step_fused_equals_unfused_and_zero_weight_is_rgb_only(gpu):
    W, H = 160, 112
    scene = make_scene(6_000, W, H, seed=11)
    cams = _cams(W, H, [(-3.0, -0.05), (0.0, 0.0), (3.0, 0.05)])
    images, ranges = _truth(gpu, scene, cams)
    start = to_torch(scene, gpu)
    start[0] = start[0] * 1.05
    start[4] = start[4] + 0.3

    def run(depths, weight, fuse, mode="residual"):
        opt = TrainOptions(n_iters=100, n_iters_warmup=3, depth_weight=weight, depth_mode=mode)
        tr = Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 20, fuse_adam=fuse, depths=depths)
        assert tr._can_fuse_adam() == fuse
        vals = [tr.train_step(i, i % 3).clone() for i in range(10)]
        dv = tr.depth_loss.values.clone() if tr.depth_loss is not None else None
        return tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.accum_grad.clone(), torch.stack(vals), dv

    for mode in ("residual", "expected"):
        a, b = run(ranges, 0.3, True, mode), run(ranges, 0.3, False, mode)
        for x, y in zip(a, b):
            assert torch.equal(x, y), mode
        assert float(a[4][0]) > 0 and float(a[4][1]) > 0  # (depth loss, pixels that counted) of the last step
    plain = run(None, 0.0, True)
    zero_w = run(ranges, 0.0, True)
    for x, y in zip(plain[:4], zero_w[:4]):
        assert torch.equal(x, y)
    assert zero_w[4] is None  # no depth-supervised step was taken
    assert not torch.equal(plain[0], a[0])  # ... and with a weight the maps do steer the fit
    # a view without a map trains on colour alone
    some = run([ranges[0], None, ranges[2]], 0.3, True)
    assert not torch.equal(some[0], a[0]) and not torch.equal(some[0], plain[0])


def test_trainer_depth_kind_z_agrees_with_range(gpu):
    """z-depth produced from a range map by the renderer's own rays converts back to that range map."""
    W, H = 250, 187
    cam = _cams(W, H, [(4.0, 0.1)])[0]
    scene = make_scene(3_000, W, H, seed=3)
    images, ranges = _truth(gpu, scene, [cam])
    ones = torch.ones(H, W, device=gpu)
    factor = z_to_range(ones, cam)  # |ray| / ray_z per pixel
    assert float(factor.min()) >= 1.0 and float(factor.max()) > 1.05
    z = (ranges[0].double() / factor.double()).float()
    p = to_torch(scene, gpu)
    tr_r = Trainer([t.clone() for t in p], [cam], images, TrainOptions(depth_weight=0.1), depths=[ranges[0]])
    tr_z = Trainer([t.clone() for t in p], [cam], images, TrainOptions(depth_weight=0.1), depths=[z], depth_kind="z")
    valid = ranges[0] > 0
    assert torch.equal(tr_z.depths[0] > 0, valid)
    err = float(((tr_z.depths[0] - tr_r.depths[0]).abs() / tr_r.depths[0].clamp_min(1e-6))[valid].max())
    print(f"z -> range round trip: max rel err {err:.2e}")
    assert err <= 4 * 2.0 ** -24  # two fp32 roundings each way
    assert tr_z._depth_inv_n == tr_r._depth_inv_n == [1.0 / int(valid.sum())]


# ------------------------------------------------------------------------------------------------------ 5. it helps
def test_depth_supervision_helps(gpu):
    """A synthetic scene (gs_scene.make_scene, 3,000 Gaussians, 160 x 112), truth images and truth range maps of five training
    views, start positions displaced along the rays of the central view by 8 % (sigma) of their range; 400 steps from the
    same seed with depth_weight 0 and 0.2 ("residual"); three held-out views.

    Measured on an MI355X (mean over the held-out views): expected-depth error 0.1824 at the start,
    0.1003 after the rgb-only fit, 0.0492 after the RGB-D fit; PSNR 27.04 dB at the start, 34.80 / 35.79 / 35.72 dB rgb-only
    over the three seeds (spread 0.99 dB), 35.11 dB RGB-D (seed 0, against 34.80)."""
    W, H = 160, 112
    scene = make_scene(3_000, W, H, seed=21)
    train_cams = _cams(W, H, [(-6.0, -0.3), (-3.0, -0.15), (0.0, 0.0), (3.0, 0.15), (6.0, 0.3)])
    held_cams = _cams(W, H, [(-4.5, -0.22), (1.5, 0.08), (4.5, 0.22)])
    images, ranges = _truth(gpu, scene, train_cams)
    held_images, held_ranges = _truth(gpu, scene, held_cams)
    start = to_torch(scene, gpu)
    noise = torch.randn(start[0].shape[0], 1, device=gpu, generator=torch.Generator(gpu).manual_seed(9))
    start[0] = start[0] * (1.0 + 0.08 * noise)  # the central camera sits at the origin: along its view rays
    steps = 400

    def evaluate(params):
        r = FrameRenderer(gpu, max_pairs=1 << 20, auto_grow=True)
        errs, psnrs = [], []
        for cam, img_t, rng_t in zip(held_cams, held_images, held_ranges):
            img, _, d, a = r.forward(*params, cam, training=False, aux=True)
            ok = (rng_t > 0) & (a >= 0.5)
            errs.append(float(((d / a.clamp_min(1e-6)) - rng_t).abs()[ok].mean()))
            psnrs.append(Trainer.psnr(img.clamp(0, 1), img_t.clamp(0, 1)))
        return float(np.mean(errs)), float(np.mean(psnrs))

    def fit(weight, seed):
        opt = TrainOptions(n_iters=steps + 1, n_iters_warmup=10, depth_weight=weight)
        tr = Trainer([t.clone() for t in start], train_cams, images, opt, max_pairs=1 << 20, depths=ranges)
        order = np.random.default_rng(seed).integers(0, len(train_cams), steps)
        for i in range(steps):
            tr.train_step(i, int(order[i]))
        return evaluate(tr.flat.params)

    err0, psnr0 = evaluate(start)
    rgb_runs = [fit(0.0, s) for s in (0, 1, 2)]
    spread = max(p for _, p in rgb_runs) - min(p for _, p in rgb_runs)
    err_rgb, psnr_rgb = rgb_runs[0]
    err_d, psnr_d = fit(0.2, 0)
    print(f"held-out expected-depth error: start {err0:.4f}, rgb only {err_rgb:.4f}, rgb-d {err_d:.4f}; PSNR: start "
          f"{psnr0:.2f}, rgb only {[round(p, 2) for _, p in rgb_runs]} (spread {spread:.3f} dB over three seeds), rgb-d {psnr_d:.2f}")
    assert math.isfinite(err_d) and math.isfinite(psnr_d)
    assert err_d < err0
    assert err_d < err_rgb
    assert psnr_d >= psnr_rgb - spread
