"""GPU tier of the loss calibration: gs_loss_l1_ssim and gs_loss_l1_ssim_weighted (gs_train.ImageLoss / WeightedImageLoss) against
the float64 truth ELEMENT BY ELEMENT, in units of each element's conditioning (tests/loss_calib_ref.py), on the images training
sees -- flat black and white backgrounds, a prediction that is all background, one that is almost the target, one that is the
target, constants, a flat half beside noise, exact ties, a zero-weight blob -- and on the pair a fit really starts from.

Asserted per case ("the loss"):
  * |g_hip - g64| <= 8 F_REF 2^-24 scale for every element; exactly +-0 where the truth and the scale are both zero;
  * the median, 99th and 99.9th percentile of that ratio <= 4 x the numpy-float32 restatement's (floored at 0.05 F_REF);
  * ssim, l1 and loss within 8 F_REF_SSIM of the value's scale plus the fp32 bound of the fixed-order sums.
Measured figures: profiles/loss_calibration.txt (every check prints its row)."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_calib_ref as lc
from gate_map_ref import weight_sums
from gs_testutil import to_torch

pytestmark = pytest.mark.gpu

K = 8.0 * lc.F_REF
K_SSIM = 8.0 * lc.F_REF_SSIM
Q_FACTOR, Q_FLOOR = 4.0, 0.05 * lc.F_REF
# The longest chain of fp32 additions between a term and a value: a thread of the streaming kernel adds its strip's 52 rows, the
# workgroup's sum takes 6 shuffle steps and 8 wave sums, and the finishing kernel one more addition per 256 workgroups, 6 shuffle
# steps and 4 wave sums.
N_TERMS = 52 + 6 + 8 + 1 + 6 + 4

# The smallest shapes at which the streaming kernel's structure is complete (a workgroup covers 52 rows x 482 flat columns, and
# 482 mod 3 = 2 rotates the channel phase of a column block): one interior pixel; one interior row and two column blocks; two
# strips; three strips with a ragged last one and two blocks; two strips and four blocks -- all three phases.
SHAPES = [(11, 11), (12, 163), (64, 80), (120, 176), (60, 484)]
CASES = [(h, w, 0.2, n) for h, w in SHAPES for n in lc.PAIR_NAMES] + [(64, 80, 1.0, n) for n in lc.PAIR_NAMES]
WEIGHTED_CASES = [(h, w, n, mp) for h, w in ((64, 80), (120, 176)) for n in ("black_bg", "late_fit", "half_flat")
                  for mp in ("blob", "soft")]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(gpu, x, y, sw, m=None):
    """Two calls into NaN-filled outputs -> (gradient, values) in numpy.  Asserts on the way what needs no tolerance: the two
    calls give identical bits, everything is written, the inputs are unchanged bit for bit."""
    from gs_train import ImageLoss, WeightedImageLoss

    h, w, _ = x.shape
    host = [x, y] + ([m] if m is not None else [])
    dev = [torch.tensor(a, device=gpu) for a in host]  # (a copy: the shared inputs are read-only)
    loss = (ImageLoss if m is None else WeightedImageLoss)(h, w, sw, gpu)
    extra = () if m is None else weight_sums(m)
    out = []
    for _ in range(2):
        loss.grad.fill_(float("nan"))
        loss.values.fill_(float("nan"))
        g = loss(*dev, *extra)
        assert g is loss.grad
        out.append((g.cpu().numpy(), loss.values.cpu().numpy()))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    for a, d in zip(host, dev):
        assert np.array_equal(_bits(a), _bits(d.cpu().numpy()))
    return out[0]


def _check(label, g, vals, ref, sw):
    """The three asserts of the module's docstring for one kernel result against ``loss_calib_ref.reference_of``'s dict."""
    sw = float(np.float32(sw))
    r = lc.ratio(g, ref["grad"], ref["scale"])
    q = lc.quantiles(r)
    lo, l1, ssim = ref["values"]
    b_lo, b_l1, b_ssim = lc.value_bounds(sw, ref["scale_ssim"], ref["scale_l1"], ref["s_abs"], lo, N_TERMS, K_SSIM)
    dv = [abs(float(vals[0]) - lo) / b_lo, abs(float(vals[1]) - l1) / b_l1 if b_l1 > 0 else float(vals[1] != 0),
          abs(float(vals[2]) - ssim) / b_ssim]
    print(f"loss-calib {lc.table_row(label, q)}   numpy-f32 " + " ".join(f"{v:7.4f}" for v in ref['q32']) +
          "   values/bound " + " ".join(f"{v:6.3f}" for v in dv))
    nothing = (ref["grad"] == 0) & (ref["scale"] == 0)
    assert not (g[nothing] != 0).any(), (label, "an element that nothing contributes to is not +-0")
    worst = np.unravel_index(np.argmax(r), r.shape)
    assert q[3] <= K, (label, "worst err / (2^-24 scale)", q[3], "at", worst, "got", float(g[worst]), "truth",
                       float(ref["grad"][worst]), "scale", float(ref["scale"][worst]))
    for a, b, name in zip(q[:3], ref["q32"][:3], lc.Q_NAMES):
        assert a <= Q_FACTOR * max(b, Q_FLOOR), (label, name, "hip", a, "numpy float32", b)
    assert max(dv) <= 1.0, (label, "loss, l1, ssim error / bound", dv, vals.tolist(), ref["values"])
    return q


@pytest.mark.parametrize("h,w,sw,name", CASES)
def test_gradient_element_by_element(gpu, h, w, sw, name):
    x, y = lc.inputs(h, w)[0][name]
    g, vals = _run(gpu, x, y, sw)
    _check(lc.case_label(h, w, name, sw, None), g, vals, lc.reference(h, w, name, sw), sw)
    if name == "equal":
        assert vals[1] == 0.0  # |x - x| sums to an exact zero


@pytest.mark.parametrize("h,w,name,mp", WEIGHTED_CASES)
def test_weighted_gradient_element_by_element(gpu, h, w, name, mp):
    (x, y), m = lc.inputs(h, w)[0][name], lc.inputs(h, w)[1][mp]
    g, vals = _run(gpu, x, y, 0.2, m)
    _check(lc.case_label(h, w, name, 0.2, mp), g, vals, lc.reference(h, w, name, 0.2, mp), 0.2)
    # out of reach of every weighted window and switched off itself: +0.0, whatever the images hold there (the neighbourhood of
    # 11 x 11 contains every element whose 21 x 21 neighbourhood has weight zero)
    far = lc.out_of_reach(m)
    assert far.sum() > 0.05 * h * w and lc.out_of_reach(m, 10).any()
    assert not _bits(g[far]).any()


@pytest.mark.parametrize("name", ["black_bg", "equal"])
def test_all_ones_weights_give_the_unweighted_bits_on_flat_images(gpu, name):
    """test_gpu_gate_map.py asserts this on noise; flat windows are where a product with 1.0f could be contracted differently."""
    for h, w in ((64, 80), (120, 176)):
        x, y = lc.inputs(h, w)[0][name]
        g, vals = _run(gpu, x, y, 0.2)
        gw, vw = _run(gpu, x, y, 0.2, lc.inputs(h, w)[1]["ones"])
        assert np.array_equal(_bits(g), _bits(gw)) and np.array_equal(_bits(vals), _bits(vw))


@pytest.mark.parametrize("name", ["black_bg", "late_fit", "half_flat"])
def test_swapped_images_give_the_same_values(gpu, name):
    """l1 and ssim are symmetric in (pred, target): the kernel's values for the swapped pair lie within the two asserted bounds of
    each other, and l1 -- |x - y| and |y - x| are the same floats, added in the same order -- agrees bit for bit."""
    h, w, sw = 64, 80, 0.2
    x, y = lc.inputs(h, w)[0][name]
    ref = lc.reference(h, w, name, sw)
    _, v = _run(gpu, x, y, sw)
    _, vs = _run(gpu, y, x, sw)
    ref_s = lc.reference_of(y, x, float(np.float32(sw)))
    bounds = [lc.value_bounds(float(np.float32(sw)), r["scale_ssim"], r["scale_l1"], r["s_abs"], r["values"][0], N_TERMS, K_SSIM)
              for r in (ref, ref_s)]
    assert _bits(v[1:2]) == _bits(vs[1:2])
    assert abs(float(v[2]) - float(vs[2])) <= bounds[0][2] + bounds[1][2]
    assert abs(float(v[0]) - float(vs[0])) <= bounds[0][0] + bounds[1][0]


def test_the_pair_training_starts_from(gpu):
    """The scene, camera and target of test_gpu_train.py::test_trainer_improves_psnr; pred is the Trainer's render before its first
    step, downloaded; truth, scale and the reference arithmetic's quantiles are computed from the downloaded arrays."""
    from gs_frame import FrameRenderer
    from gs_scene import make_camera, make_scene
    from gs_train import TrainOptions, Trainer

    W, H = 160, 128
    scene, cam = make_scene(3000, W, H, seed=9), make_camera(W, H)
    gt = to_torch(scene, gpu)
    target, _ = FrameRenderer(gpu, max_pairs=1 << 16).forward(*gt, cam)
    target = target.clone()
    rng = np.random.default_rng(1)
    start = [t.clone() for t in gt]
    start[4] = start[4] + torch.from_numpy(rng.normal(0, 1.0, tuple(start[4].shape)).astype(np.float32)).to(gpu)
    start[3] = start[3] + torch.from_numpy(rng.normal(0, 0.5, tuple(start[3].shape)).astype(np.float32)).to(gpu)
    tr = Trainer(start, [cam], [target], TrainOptions(n_iters=400, n_iters_warmup=10), max_pairs=1 << 16)
    img0, _ = tr.renderer.forward(*tr.flat.params, cam)
    x, y = np.ascontiguousarray(img0.cpu().numpy()[:H, :W]), np.ascontiguousarray(target.cpu().numpy()[:H, :W])
    assert x.shape == (H, W, 3) and x.dtype == np.float32 and np.abs(x - y).max() > 0.05
    ref = lc.reference_of(x, y, float(np.float32(0.2)))
    top = np.abs(ref["grad"]).max()
    print(f"rendered pair: {np.mean(np.abs(ref['grad']) < 1e-3 * top):.2f} of the gradient below 1e-3 of its largest entry; "
          f"numpy float32 max error / max {np.abs(ref['grad32'] - ref['grad']).max() / top:.2e}")
    g, vals = _run(gpu, x, y, 0.2)
    _check(f"{H}x{W} w=0.2 rendered step 0", g, vals, ref, 0.2)


@pytest.mark.parametrize("h,w", [(10, 40), (40, 10)])
def test_ssim_refuses_an_image_no_larger_than_its_window(gpu, h, w):
    """Both entry points: return code, message and untouched outputs with a weight; with weight 0 the same sizes succeed and give
    the L1 gradient exactly."""
    from gaussian import _lib
    from gs_train import ImageLoss, WeightedImageLoss

    rng = np.random.default_rng(h)
    x = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    y = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    y[::3, ::4] = x[::3, ::4]
    m = np.ones((h, w), np.float32)
    m[2:5, 3:9] = 0.0
    xd, yd, md = (torch.from_numpy(a).to(gpu) for a in (x, y, m))
    ws = torch.zeros(_lib.gs_loss_workspace_bytes(h, w), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    sums = weight_sums(m)
    assert sums[1] == 0.0
    for weighted in (False, True):
        grad = torch.full((h, w, 3), 7.0, device=gpu)
        vals = torch.full((3,), 7.0, device=gpu)
        tail = (grad.data_ptr(), vals.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        call = (lambda sw: _lib.gs_loss_l1_ssim_weighted(xd.data_ptr(), yd.data_ptr(), md.data_ptr(), h, w, sw, C.c_double(sums[0]),
                                                         C.c_double(float(h * w)), *tail)) if weighted else \
            (lambda sw: _lib.gs_loss_l1_ssim(xd.data_ptr(), yd.data_ptr(), h, w, sw, *tail))
        assert call(0.1) == -1 and b"11x11 window" in _lib.gs_last_error()
        torch.cuda.synchronize()
        assert (grad == 7.0).all() and (vals == 7.0).all()
        obj = (WeightedImageLoss if weighted else ImageLoss)(h, w, 0.1, gpu)
        obj.grad.fill_(7.0)
        obj.values.fill_(7.0)
        with pytest.raises(RuntimeError, match="11x11 window"):
            obj(xd, yd, md, *sums) if weighted else obj(xd, yd)
        assert (obj.grad == 7.0).all() and (obj.values == 7.0).all()
        assert call(0.0) == 0
        mm = m[:, :, None] if weighted else 1.0
        a = np.float32(1.0 / (3.0 * (sums[0] if weighted else h * w)))
        want = (a * mm * np.sign(x - y)).astype(np.float32)
        want[np.broadcast_to(np.asarray(mm) == 0, want.shape)] = 0.0  # (+0.0 under a zero weight, whatever the sign)
        got = grad.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
        l1 = float((mm * np.abs(x.astype(np.float64) - y)).sum() * a)
        v = vals.cpu().numpy()
        assert abs(v[1] - l1) <= (N_TERMS + 2) * lc.U * l1 and v[2] == 0.0 and abs(v[0] - l1) <= (N_TERMS + 4) * lc.U * l1
