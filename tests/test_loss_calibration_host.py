"""CPU tier of the loss calibration (tests/loss_calib_ref.py): the float64 truth against torch autograd, the conditioning scale
against the numpy-float32 restatement of the same formulas (F_REF), and the properties of the scale and of the inputs that the GPU
tier (tests/test_gpu_loss_calibration.py) relies on.  profiles/loss_calibration.txt holds the table this file measures."""
import os

import numpy as np
import pytest
import torch

import loss_calib_ref as lc
from test_train_ref import torchmetrics_ssim_restated

SIZE, BIG = (64, 80), (120, 176)
U64 = 2.0 ** -53


@pytest.mark.parametrize("h,w,sw,name", [SIZE + (sw, n) for sw in (0.2, 1.0) for n in lc.PAIR_NAMES] + [BIG + (0.2, "late_fit")])
def test_truth_matches_autograd_of_restated_torchmetrics(h, w, sw, name):
    """The truth is the project's float64 restatement; on these images too it is what torch.autograd makes of the literal
    torchmetrics restatement -- within 64 unit roundoffs of float64 per unit of the scale, which also says that the scale covers
    the one place where float64 itself is not smooth (a clamp decided by rounding noise on a flat window)."""
    x, y = lc.inputs(h, w)[0][name]
    ref = lc.reference(h, w, name, sw)
    sw = float(np.float32(sw))  # (the truth is taken at the fp32 value of the weight)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64)
    l1_t = (xt - yt).abs().mean()
    ssim_t = torchmetrics_ssim_restated(xt.unsqueeze(0).permute(0, 3, 1, 2), yt.unsqueeze(0).permute(0, 3, 1, 2))
    loss_t = (1 - sw) * l1_t + sw * (1.0 - ssim_t)
    loss_t.backward()
    lo, l1, ssim = ref["values"]
    assert abs(l1 - l1_t.item()) < 1e-14 and abs(ssim - ssim_t.item()) < 1e-12 and abs(lo - loss_t.item()) < 1e-12
    err = np.abs(ref["grad"] - xt.grad.numpy())
    assert (err <= 64 * U64 * ref["scale"]).all(), float((err / (U64 * ref["scale"] + 1e-300)).max())


def test_scale_bounds_the_reference_arithmetic():
    """F_ref: the numpy-float32 restatement's error never exceeds F_REF x 2^-24 x scale, element by element, on any pair under
    any weight map; its SSIM value stays within F_REF_SSIM of the value's scale.  The measured figures stand beside the recorded
    ones in profiles/loss_calibration.txt."""
    text, f_ref, f_ssim = lc.host_report()
    print(text)
    for c in lc.HOST_CASES:
        r = lc.reference(*c)
        assert np.isfinite(r["ratio32"]).all(), c  # (inf: an error where the scale is zero)
        assert r["q32"][3] <= lc.F_REF, (c, r["q32"])
        assert r["ratio32_ssim"] <= lc.F_REF_SSIM, (c, r["ratio32_ssim"])
    assert 0.5 * lc.F_REF <= f_ref <= lc.F_REF and 0.5 * lc.F_REF_SSIM <= f_ssim <= lc.F_REF_SSIM  # recorded, not invented
    assert lc.AMBIGUOUS >= 8 * lc.F_REF
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loss_calibration.txt")
    with open(path) as f:
        recorded = f.read()
    assert f"recorded F_REF = {lc.F_REF}" in recorded and f"recorded F_REF_SSIM = {lc.F_REF_SSIM}" in recorded


def test_no_tensor_max_criterion_describes_these_images():
    """Why the element-wise standard: on the flat pairs most of the gradient lies far below the tensor's largest entry, and the
    reference arithmetic itself misses the 2e-5 x max of test_loss_matches_oracle on two of them."""
    share, rel = {}, {}
    for name in lc.PAIR_NAMES:
        r = lc.reference(*SIZE, name, 0.2)
        top = np.abs(r["grad"]).max()
        share[name] = float(np.mean(np.abs(r["grad"]) < 1e-3 * top))
        rel[name] = float(np.abs(r["grad32"] - r["grad"]).max() / top)
    print(share, rel)
    assert share["noise"] < 0.05 and rel["noise"] < 2e-6
    assert min(share[n] for n in ("black_bg", "white_bg", "late_fit", "ties")) > 0.25
    assert rel["white_bg"] > 2e-5 and rel["late_fit"] > 2e-5


@pytest.mark.parametrize("mp", (None,) + lc.WEIGHT_NAMES)
def test_scale_is_positive_wherever_the_truth_is_not_zero(mp):
    for name in lc.PAIR_NAMES:
        for sw in (0.2,) if mp else (0.2, 1.0):
            r = lc.reference(*SIZE, name, sw, mp)
            assert (r["scale"] >= 0).all() and np.isfinite(r["scale"]).all()
            assert (r["scale"][r["grad"] != 0] > 0).all(), (name, sw, mp)
            assert r["scale_ssim"] > 0 and (r["scale_l1"] > 0) == (name != "equal")
    # ... and is zero where nothing is computed: under a zero weight out of reach of every weighted window, and on an all-black
    # pair, whose every term is an exact zero
    if mp == "blob":
        m = lc.inputs(*SIZE)[1]["blob"]
        far = lc.out_of_reach(m)
        assert far.any() and not lc.reference(*SIZE, "late_fit", 0.2, "blob")["scale"][far].any()
    black = np.zeros(SIZE + (3,), np.float32)
    sc, sc_ssim, sc_l1, _ = lc.scale(black, black, 0.2)
    assert not sc.any() and sc_l1 == 0 and sc_ssim > 0


def test_scale_depends_on_the_arrays_alone():
    """No hidden dependence on the kind of content: the scale commutes with what the formulas commute with -- flips, the
    transposition, a permutation of the channels, all exactly up to the order of float64 sums -- and is local: more than 10 pixels
    away from the discs, black_bg's scale is that of an all-black pair and white_bg's that of an all-white one.  Exchanging the
    constant of a flat region between 0 and 1 leaves the L1 part alone (ssim_weight 0: bit for bit) and changes the SSIM part, as
    c1 and c2 say it must: all-white windows have a conditioning, all-black ones are exact zeros."""
    P = lc.inputs(*SIZE)[0]
    x, y = P["late_fit"]
    sc = lc.scale(x, y, 0.2)[0]
    for f in (lambda a: a[::-1], lambda a: a[:, ::-1], lambda a: np.swapaxes(a, 0, 1), lambda a: a[:, :, [2, 0, 1]]):
        got = lc.scale(np.ascontiguousarray(f(x)), np.ascontiguousarray(f(y)), 0.2)[0]
        assert np.allclose(got, f(sc), rtol=1e-9, atol=0)
    for name, c in (("black_bg", 0.0), ("white_bg", 1.0)):
        flat = np.full(SIZE + (3,), c, np.float32)
        px, py = P[name]
        far = lc.out_of_reach(np.any(py != np.float32(c), axis=2), 10)  # (window and adjoint: 5 + 5)
        assert far.sum() > 50
        a, b = lc.scale(px, py, 0.2)[0], lc.scale(flat, flat, 0.2)[0]
        assert np.allclose(a[far], b[far], rtol=1e-9, atol=0)
        assert bool(b.any()) == (c == 1.0)
    l1_black, l1_white = lc.scale(*P["black_bg"], 0.0)[0], lc.scale(*P["white_bg"], 0.0)[0]
    assert np.array_equal(l1_black, l1_white) and l1_black.any()


def test_inputs_are_deterministic_and_what_they_claim():
    for h, w in ((11, 11), (12, 163), SIZE):
        a, b = lc.pairs(h, w), lc.pairs(h, w)
        assert tuple(a) == lc.PAIR_NAMES
        for name in a:
            for u, v in zip(a[name], b[name]):
                assert u.dtype == np.float32 and u.shape == (h, w, 3) and np.array_equal(u.view(np.uint32), v.view(np.uint32))
                assert u.min() >= 0 and u.max() <= 1
        ma, mb = lc.weight_maps(h, w), lc.weight_maps(h, w)
        assert tuple(ma) == lc.WEIGHT_NAMES and all(np.array_equal(ma[k], mb[k]) and ma[k].dtype == np.float32 for k in ma)
    P, M = lc.inputs(*SIZE)
    h, w = SIZE
    assert not P["black_bg"][0].any() and (P["white_bg"][0] == 1).all() and P["black_bg"][1].any()
    assert np.array_equal(P["equal"][0], P["equal"][1]) and np.ptp(P["equal"][0]) > 0.5
    assert np.ptp(P["const"][0]) == 0 and np.ptp(P["const"][1]) == 0 and P["const"][0][0, 0, 0] != P["const"][1][0, 0, 0]
    hx, hy = P["half_flat"]
    assert np.ptp(hx[:, :w // 2]) == 0 and np.array_equal(hx[:, :w // 2], hy[:, :w // 2]) and np.ptp(hx[:, w // 2:]) > 0.5
    tx, ty = P["ties"]
    tied = (tx == ty).all(axis=2) & ty.any(axis=2)
    assert 0.02 * h * w / 10 < tied.sum() and np.array_equal(tx[~tied], P["black_bg"][0][~tied])
    lx, ly = P["late_fit"]
    flat = lc.out_of_reach((ly != 1).any(axis=2), 3)  # (three passes of a 3 x 3 blur)
    assert 0 < np.abs(lx - ly).max() < 0.5 and flat.mean() > 0.3 and (lx[flat] == 1).all()  # the background stays exactly flat
    zero = M["blob"] == 0
    assert 0.15 < zero.mean() < 0.35 and zero[:, 0].any() and not zero[:, -1].any()  # a quarter, touching the left border
    assert np.array_equal(M["soft"] == 0, zero) and M["soft"].max() <= 1 and M["soft"][~zero].min() > 0 and (M["ones"] == 1).all()
