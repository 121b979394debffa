"""GPU tier of the per-view exposure kernels (gs_exposure_apply / gs_exposure_backward, csrc/exposure.hip) against the
restatement of tests/exposure_ref.py: the two maps bit for bit, the six sums inside the bound of a fixed-order double sum, the
closed form of the L1 chain from the inputs alone, the device Adam step against Python floats, and a Trainer step on a view
with an identity exposure bit for bit the step without one.  include/gs_abi.h states the contracts."""
import math

import numpy as np
import pytest
import torch

import exposure_ref as X

pytestmark = pytest.mark.gpu

# 1 x 1: one tail pixel; 5 x 7 and 31 x 33: no multiple of four, under and over one workgroup; 160 x 120: whole workgroups;
# 1080 x 1920: 2,025 rows for the last workgroup (there is no grid cap: more rows than its 1,024 threads)
SIZES = [(1, 1), (5, 7), (31, 33), (120, 160), (1080, 1920)]
_CASES = {}


def _case(H, W):
    """(image in [0, 1], gradient with exact zeros and both signs, the restatement's answers for GAIN* / BIAS*): once per
    size, never modified."""
    if (H, W) not in _CASES:
        rng = np.random.default_rng(1000 * H + W)
        img = rng.random((H, W, 3), dtype=np.float32)
        grad = rng.normal(size=(H, W, 3)).astype(np.float32)
        grad[rng.random(grad.shape) < 0.25] = 0.0
        if H * W == 1:
            grad[0, 0] = (0.5, 0.0, -2.0)
        num = X.numbers(X.GAIN_STAR, X.BIAS_STAR)
        _CASES[(H, W)] = (img, grad, num, X.apply(img, num), X.backward(img, grad, num))
    return _CASES[(H, W)]


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_pair_against_the_restatement(gpu, H, W):
    from gs_exposure import Exposure

    img, grad, num, out_ref, (g_ref, sums, bound) = _case(H, W)
    ex = Exposure(H, W, gpu, num[0:3], num[3:6])
    ti = torch.from_numpy(img).to(gpu)
    ex.out.fill_(float("nan"))
    out = ex.apply(ti)
    assert _bits(out) == out_ref.tobytes()
    runs = []
    for _ in range(2):
        g = torch.from_numpy(grad).to(gpu)
        ex.grad.fill_(float("nan"))
        assert ex.backward(ti, g) is g
        runs.append((_bits(g), _bits(ex.grad)))
        assert runs[-1][0] == g_ref.tobytes()
    assert runs[0] == runs[1]  # bitwise repeatable
    got = ex.grad.cpu().numpy().astype(np.float64)
    err = np.abs(got - sums)
    print(f"exposure {W}x{H}: sums {got.tolist()} err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), (got, sums, bound)
    assert _bits(ex.numbers) == num.tobytes() and _bits(ti) == img.tobytes()  # fixed: nothing else is written
    # the identity: out is image's bits, grad unchanged bit for bit
    ident = Exposure(H, W, gpu)
    assert _bits(ident.apply(ti)) == img.tobytes()
    g = torch.from_numpy(grad).to(gpu)
    ident.backward(ti, g)
    assert _bits(g) == grad.tobytes()
    gain, bias = ident.values()
    assert gain.tolist() == [1, 1, 1] and bias.tolist() == [0, 0, 0] and gain.dtype == np.float64


def test_refusals_through_the_class(gpu):
    from gs_exposure import Exposure

    ex = Exposure(12, 16, gpu)
    good = torch.zeros(12, 16, 3, device=gpu)
    for bad in (torch.zeros(16, 12, 3, device=gpu), torch.zeros(12, 16, 3), torch.zeros(12, 16, 3, dtype=torch.float64, device=gpu),
                torch.zeros(12, 16, 6, device=gpu)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="contiguous float32 HIP tensor"):
            ex.apply(bad)
        with pytest.raises(RuntimeError, match="contiguous float32 HIP tensor"):
            ex.backward(good, bad)
    with pytest.raises(RuntimeError, match="alias"):
        ex.backward(good, good)
    with pytest.raises(ValueError):
        ex.free(-1e-3, 1e-3)


@pytest.mark.parametrize("H,W", [(5, 7), (31, 33), (120, 160)])
@pytest.mark.parametrize("weighted", [False, True])
def test_l1_chain_has_its_closed_form(gpu, H, W, weighted):
    """ssim_weight 0: apply -> gs_loss_l1_ssim -> backward gives dL/dgain_c = sum_p sign(I' - T) I / (3 H W) and dL/dbias_c =
    sum_p sign(I' - T) / (3 H W), evaluated here in float64 from the inputs alone (I' is the restatement's: the same bits, and
    the sign of a float32 difference is the sign of the difference).  Bound: the fixed-order double sum's n 2^-53 sum|term|,
    the sum's one rounding to float32, and the float32 rounding of the per-pixel constant 1 / (3 H W) (2^-24 relative).  The
    weighted loss with an all-ones map is the same function."""
    from gs_exposure import Exposure
    from gs_train import ImageLoss, WeightedImageLoss

    img, _, num, out_ref, _ = _case(H, W)
    tgt = np.random.default_rng(7 * H + W).random((H, W, 3), dtype=np.float32)
    tgt[::2, ::3] = out_ref[::2, ::3]  # exact zeros of the gradient
    ex = Exposure(H, W, gpu, num[0:3], num[3:6])
    ti, tt = torch.from_numpy(img).to(gpu), torch.from_numpy(tgt).to(gpu)
    if weighted:
        loss = WeightedImageLoss(H, W, 0.0, gpu)
        g = loss(ex.apply(ti), tt, torch.ones(H, W, device=gpu), float(H * W), float(max(H - 10, 0) * max(W - 10, 0)))
    else:
        loss = ImageLoss(H, W, 0.0, gpu)
        g = loss(ex.apply(ti), tt)
    ex.backward(ti, g)
    sign = np.sign(out_ref.astype(np.float64) - tgt.astype(np.float64)).reshape(-1, 3)
    I = img.astype(np.float64).reshape(-1, 3)
    n, c = H * W, 1.0 / (3.0 * H * W)
    want = np.asarray([c * math.fsum(sign[:, k] * I[:, k]) for k in range(3)] + [c * math.fsum(sign[:, k]) for k in range(3)])
    mags = np.asarray([c * math.fsum(np.abs(sign[:, k]) * I[:, k]) for k in range(3)]
                      + [c * math.fsum(np.abs(sign[:, k])) for k in range(3)])
    bound = n * 2.0 ** -53 * mags + 2.0 * 2.0 ** -24 * np.abs(want) + 2.0 ** -149
    got = ex.grad.cpu().numpy().astype(np.float64)
    print(f"exposure L1 chain {W}x{H} weighted={weighted}: {got.tolist()} vs {want.tolist()}, err / bound "
          f"{(np.abs(got - want) / bound).max():.3f}")
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    assert (sign == 0).any() and np.abs(want[0:3]).min() > 0


@pytest.mark.parametrize("H,W", [(31, 33), (120, 160)])
def test_chain_rule_identity_with_ssim_on(gpu, H, W):
    """With SSIM there is no closed form: the six gradients are the restatement's sums of the loss kernel's OWN gradient map,
    and the map that leaves is that map scaled, bit for bit."""
    from gs_exposure import Exposure
    from gs_train import ImageLoss

    img, _, num, _, _ = _case(H, W)
    tgt = np.random.default_rng(11 * H + W).random((H, W, 3), dtype=np.float32)
    ex = Exposure(H, W, gpu, num[0:3], num[3:6])
    ti, tt = torch.from_numpy(img).to(gpu), torch.from_numpy(tgt).to(gpu)
    g = ImageLoss(H, W, 0.2, gpu)(ex.apply(ti), tt)
    gp = g.cpu().numpy().copy()
    ex.backward(ti, g)
    g_ref, sums, bound = X.backward(img, gp, num)
    assert _bits(g) == g_ref.tobytes()
    got = ex.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got - sums) <= bound).all() and np.abs(sums).min() > 0


def test_device_adam_follows_the_python_floats(gpu):
    """20 steps on recorded gradients: each step's new float32 numbers equal the restatement's step from the numbers and the
    float32 gradients the device held, the state carried in Python floats.  Where the two libraries' pow or sqrt differ in a
    last double bit that shows in a float32, one float32 ulp is allowed there and the step printed."""
    from gs_exposure import Exposure

    H, W = 31, 33
    img, _, num, _, _ = _case(H, W)
    rng = np.random.default_rng(3)
    ex = Exposure(H, W, gpu, num[0:3], num[3:6])
    opts = X.default_opts(lr_gain=1e-2, lr_bias=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    ex.free(opts["lr_gain"], opts["lr_bias"], (opts["beta1"], opts["beta2"]), opts["eps"])
    assert ex.is_free
    ti = torch.from_numpy(img).to(gpu)
    state, prev, off = X.new_state(), num.astype(np.float32), []
    for k in range(20):
        g = rng.normal(size=(H, W, 3)).astype(np.float32) * np.float32(10.0 ** rng.uniform(-4, 0))
        opts["lr_scale"] = 0.97 ** k
        ex.backward(ti, torch.from_numpy(g).to(gpu), lr_scale=opts["lr_scale"])
        g6 = ex.grad.cpu().numpy()
        now = ex.numbers.cpu().numpy()
        want = np.asarray(X.step(state, prev, g6, opts), np.float32)
        if now.tobytes() != want.tobytes():
            ulps = np.abs(now.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            off.append((k, ulps.tolist()))
            assert ulps.max() <= 1, (k, now, want)
        assert (now != prev).all()  # every number moved
        prev = now
    print(f"exposure device Adam: steps off by one float32 ulp: {off if off else 'none'}")
    st = ex._fit.state.cpu().numpy()
    assert st[12] == 20.0 == state["steps"]
    assert np.allclose(st[0:6], state["m"], rtol=1e-12, atol=0) and np.allclose(st[6:12], state["v"], rtol=1e-12, atol=0)
    # a raised skip flag: state and numbers untouched bit for bit; the map is still scaled and the gradients still formed
    flag = torch.ones(1, dtype=torch.int64, device=gpu)
    before = (_bits(ex.numbers), _bits(ex._fit.state))
    g = rng.normal(size=(H, W, 3)).astype(np.float32)
    tg = torch.from_numpy(g).to(gpu)
    ex.grad.zero_()
    ex.backward(ti, tg, skip_flag=flag.data_ptr())
    assert (_bits(ex.numbers), _bits(ex._fit.state)) == before
    assert _bits(tg) == X.backward(img, g, prev)[0].tobytes() and ex.grad.abs().min() > 0
    flag.zero_()
    ex.backward(ti, torch.from_numpy(g).to(gpu), skip_flag=flag.data_ptr())
    assert _bits(ex.numbers) != before[0] and float(ex._fit.state[12]) == 21.0
    # rate 0: the step counts and the numbers stay
    ex.free(0.0, 0.0)
    held = _bits(ex.numbers)
    ex.backward(ti, torch.from_numpy(g).to(gpu))
    assert _bits(ex.numbers) == held and float(ex._fit.state[12]) == 1.0
    ex.fix()
    assert not ex.is_free


# ------------------------------------------------------------------------------------------------------------ the Trainer
def _trainer_state(tr):
    return [_bits(tr.flat.flat_param), _bits(tr.optimizer.exp_avg), _bits(tr.optimizer.exp_avg_sq)]


@pytest.mark.parametrize("kind", ["plain", "weighted", "depth"])
def test_identity_exposure_leaves_the_training_step_bit_for_bit(gpu, kind):
    """Three steps on one view: without an exposure, with a fixed identity exposure, and with an identity exposure freed at
    rate 0 -- parameters and both moments bit for bit equal, and so are the loss values.  Plain, weighted and depth-supervised
    views (the fused step, its aux variant)."""
    from gs_frame import FrameRenderer
    from gs_testutil import aux_case, to_torch
    from gs_train import TrainOptions, Trainer

    W, H = 96, 64
    scene, cam = aux_case(4000, W, H, seed=31)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False)
    img, _, d, a = r.forward(*params, cam, training=False, aux=True)
    target = (img * 0.8 + 0.05).contiguous().clone()
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3) * 1.02, torch.zeros_like(d)).contiguous().clone()
    wmap = None
    if kind == "weighted":
        wmap = torch.ones(H, W, device=gpu)
        wmap[10:30, 20:50] = 0.25
    opt = TrainOptions(n_iters_warmup=1, depth_weight=0.2 if kind == "depth" else 0.0)

    def run(mode):
        kw = dict(max_pairs=1 << 19, depths=[rng] if kind == "depth" else None, weights=[wmap] if wmap is not None else None)
        if mode != "none":
            kw["exposures"] = {0: ((1, 1, 1), (0, 0, 0))}
        tr = Trainer([p.detach().clone() for p in params], [cam], [target], opt, **kw)
        assert bool(tr._exposure) == (mode != "none")
        if mode == "free":
            tr.free_exposure(0, 0.0, 0.0)
        vals = [_bits(tr.train_step(i, 0)) for i in range(1, 4)]
        if mode != "none":
            gain, bias = tr.exposure(0)
            assert gain.tolist() == [1, 1, 1] and bias.tolist() == [0, 0, 0]
            assert tr._exposure[0].grad.abs().max() > 0  # the six gradients were formed
        else:
            assert tr.exposure(0) is None
        return _trainer_state(tr), vals, tr

    base, base_vals, tr0 = run("none")
    moved = float((tr0.flat.params[4] - params[4]).abs().max())
    assert moved > 0
    for mode in ("fixed", "free"):
        got, vals, tr = run(mode)
        assert got == base and vals == base_vals, mode
    # a non-identity exposure is a different step, and test() stays uncompensated
    tr = Trainer([p.detach().clone() for p in params], [cam], [target], opt, max_pairs=1 << 19,
                 depths=[rng] if kind == "depth" else None, weights=[wmap] if wmap is not None else None,
                 exposures={0: ((0.8, 0.8, 0.8), (0.05, 0.05, 0.05))})
    v = tr.train_step(1, 0).clone()
    assert _bits(v) != base_vals[0] and float(v[1]) < float(np.frombuffer(base_vals[0], np.float32)[1])
    shown = tr.test(0)["image"]
    assert float((shown - img).abs().max()) < 0.05  # the map's own radiometry, not the target's
    tr.add_view(cam, target, rng if kind == "depth" else None, weight=wmap, exposure=((0.9, 0.9, 0.9), (0, 0, 0)))
    assert sorted(tr._exposure) == [0, 1]
    tr.remove_view(0)
    assert sorted(tr._exposure) == [0] and tr.exposure(0)[0].tolist() == [float(np.float32(0.9))] * 3
