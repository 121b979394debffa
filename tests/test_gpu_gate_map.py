"""GPU tier of the gate carried into seeding and mapping: gs_track_gate_mask (gs_train.GateMask) bit for bit against the
float32 statement of tests/gate_map_ref.py on the inputs of the gated tracking loss's tests; gs_loss_l1_ssim_weighted
(gs_train.WeightedImageLoss) against ImageLoss (all-ones weights: bitwise) and against the float64 helper at the tolerances of
test_gpu_train.py::test_loss_matches_oracle; the occluder frame of tests/test_gpu_track_gate.py as a keyframe -- what the gate
removes, what seeding then selects, and what 30 mapping steps do to the map with and without the gate."""
import numpy as np
import pytest
import torch

from gate_map_ref import gate_mask_ref, interior, weight_sums, weighted_l1_ssim_loss
from track_gate_ref import crafted_inputs, powers_and_zeros
from track_ref import ALPHA_MIN, LOSS_CASES, loss_inputs, measured

pytestmark = pytest.mark.gpu

_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(H, W, seed):
    """The numpy inputs of a size, computed once, never modified."""
    if (H, W) not in _CACHE:
        _CACHE[(H, W)] = loss_inputs(H, W, seed)
    return _CACHE[(H, W)]


def _run_mask(gpu, x, k_d, k_c, floor_d=0.0, floor_c=0.0, couple=True, with_range=True):
    """Two calls into NaN-filled outputs -> (range or None, weight, values) in numpy; asserts the runs are bitwise equal and
    everything was written."""
    from gs_train import GateMask

    I, D, A, T, z = x
    H, W = A.shape
    t = [torch.from_numpy(a).to(gpu) for a in x]
    gm = GateMask(H, W, ALPHA_MIN, k_d, k_c, floor_d, floor_c, couple, gpu)
    runs = []
    for _ in range(2):
        for o in (gm.range, gm.weight, gm.values):
            o.fill_(float("nan"))
        rng, wgt = gm(t[0], t[1], t[2], t[3], t[4] if with_range else None)
        assert (rng is gm.range) == with_range and wgt is gm.weight
        runs.append([o.clone() for o in (gm.range, gm.weight, gm.values)])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # bitwise repeatable
    rng, wgt, vals = (o.cpu().numpy() for o in runs[0])
    assert not np.isnan(wgt).any() and not np.isnan(vals).any()  # fully written
    if with_range:
        assert not np.isnan(rng).any()
    else:
        assert np.isnan(rng).all()  # no range map: `range` is left alone
    return (rng if with_range else None), wgt, vals


def _check_mask(gpu, x, k_d, k_c, floor_d=0.0, floor_c=0.0, couple=True, with_range=True, tag=""):
    """The kernel against the helper: both maps bit for bit, the eight values exactly; m_d, m_c, n_d those of a
    GatedTrackLoss call on the same inputs.  -> (range, weight, values, the helper's gate dict)."""
    from gs_train import GatedTrackLoss

    I, D, A, T, z = x
    H, W = A.shape
    rng, wgt, vals = _run_mask(gpu, x, k_d, k_c, floor_d, floor_c, couple, with_range)
    want_rng, want_wgt, want_vals, g = gate_mask_ref(I, D, A, T, z if with_range else None, ALPHA_MIN, k_d, k_c, floor_d, floor_c,
                                                     couple)
    print(f"{tag}: values {vals.tolist()}")
    if with_range:
        assert np.array_equal(_bits(rng), _bits(want_rng))  # (+0.0 where removed or unmeasured, the input's bits elsewhere)
    assert np.array_equal(_bits(wgt), _bits(want_wgt))
    assert np.array_equal(_bits(vals), _bits(want_vals)), (vals, want_vals)
    assert vals[0] == vals[1] + vals[2] and vals[3] == wgt.sum(dtype=np.float64)
    assert vals[4] == wgt[interior(H, W)].sum(dtype=np.float64)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    gl = GatedTrackLoss(H, W, ALPHA_MIN, 0.8, 1.3, k_d, k_c, floor_d, floor_c, couple, gpu)
    gl(t[0], t[1], t[2], t[3], t[4] if with_range else None, 0.37 / (H * W))
    assert np.array_equal(_bits(gl.values.cpu().numpy()[5:8]), _bits(vals[5:8]))
    return rng, wgt, vals, g


# ------------------------------------------------------------------------------------------------------ 1. the mask kernel
@pytest.mark.parametrize("couple", [True, False])
@pytest.mark.parametrize("H,W,seed", LOSS_CASES)
def test_mask_is_the_gates_decision_bit_for_bit(gpu, H, W, seed, couple):
    """k_d = k_c = 1.5, floors 0, on the inputs of test_gpu_track_gate.py (30 % of z unmeasured in each of the four ways, A
    straddling alpha_min): every pixel of both maps and all eight values; each gate cuts something and keeps something."""
    x = _inputs(H, W, seed)
    I, D, A, T, z = x
    rng, wgt, vals, g = _check_mask(gpu, x, 1.5, 1.5, couple=couple, tag=f"mask {W}x{H} couple={couple}")
    covered, meas = A >= np.float32(ALPHA_MIN), measured(z)
    assert 0 < vals[2] < vals[0] and 0 < (wgt == 0).sum() < covered.sum()
    # a pixel the map does not cover keeps its range and has weight 1
    assert np.all(wgt[~covered] == 1) and np.array_equal(_bits(rng[~covered & meas]), _bits(z[~covered & meas]))
    assert not _bits(rng[~meas]).any()  # <= 0, inf, NaN: written as +0.0
    if couple:
        assert np.all(wgt[covered & meas & (rng == 0)] == 0)  # a pixel that lost its range lost its colour


@pytest.mark.parametrize("H,W,seed", LOSS_CASES[:3])
def test_mask_without_a_range_map_and_with_the_gates_off(gpu, H, W, seed):
    x = _inputs(H, W, seed)
    I, D, A, T, z = x
    _, wgt, vals, _ = _check_mask(gpu, x, 1.5, 1.5, with_range=False, tag=f"mask {W}x{H} RGB only")
    assert vals[0] == vals[1] == vals[2] == 0 and vals[5] == 0 and vals[7] == 0 and 0 < (wgt == 0).sum()
    for k_d, k_c in ((0.0, 0.0), (-1.0, -2.5)):  # both k <= 0: the measured input, all ones
        rng, wgt, vals, _ = _check_mask(gpu, x, k_d, k_c, tag=f"mask {W}x{H} gates off")
        meas = measured(z)
        assert np.array_equal(_bits(rng), _bits(np.where(meas, z, np.float32(0)))) and np.all(wgt == 1)
        assert vals[0] == vals[1] == meas.sum() and vals[2] == 0 and vals[3] == H * W


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64)])
def test_mask_on_the_crafted_sets(gpu, H, W):
    """The sets test_gpu_track_gate.py crafts for the loss: every residual equal; median zero with and without a floor; a NaN
    and an inf outside the sets; set sizes 0, 1 and 2."""
    n = H * W
    # every residual equal: median 1, nothing removed
    rng, wgt, vals, _ = _check_mask(gpu, crafted_inputs(H, W, np.ones(n)), 1.5, 0.0, tag=f"crafted equal {W}x{H}")
    assert vals[5] == 1.0 and vals[7] == n and vals[2] == 0 and vals[3] == n and np.all(rng == 1)
    # median zero: only the exact zeros keep their range; a floor of 0.3 admits 0.25 as well
    resid = np.where(np.arange(n) % 5 < 3, 0.0, np.where(np.arange(n) % 5 == 3, 0.25, 0.5)).astype(np.float32)
    np.random.default_rng(3).shuffle(resid)
    x = crafted_inputs(H, W, resid)
    rng, wgt, vals, _ = _check_mask(gpu, x, 1.5, 0.0, tag=f"crafted median 0 {W}x{H}")
    assert vals[5] == 0.0 and vals[1] == (resid == 0).sum() and np.array_equal(rng.reshape(-1) != 0, resid == 0)
    assert np.array_equal(wgt.reshape(-1) == 1, resid == 0)  # coupled: the rejected pixels lose their colour
    rng, wgt, vals, _ = _check_mask(gpu, x, 1.5, 0.0, floor_d=0.3, tag=f"crafted median 0, floor 0.3 {W}x{H}")
    assert vals[5] == 0.0 and vals[1] == (resid <= 0.25).sum() and np.array_equal(rng.reshape(-1) != 0, resid <= 0.25)
    # a NaN and an inf in D at covered, measured pixels: outside S_d, so the depth term does not count there -- the range
    # goes -- but the coupling does not reach them: their colour weight stays
    I, D, A, T, z = crafted_inputs(H, W, powers_and_zeros(n))
    D = D.copy()
    D.reshape(-1)[5], D.reshape(-1)[n - 2] = np.nan, np.inf
    rng, wgt, vals, _ = _check_mask(gpu, (I, D, A, T, z), 1.5, 0.0, tag=f"crafted NaN / inf {W}x{H}")
    assert vals[7] == n - 2 and not rng.reshape(-1)[[5, n - 2]].any() and np.all(wgt.reshape(-1)[[5, n - 2]] == 1)
    # set sizes 0, 1, 2 (every other pixel alternately uncovered and unmeasured)
    for n_d in (0, 1, 2):
        chosen = np.random.default_rng(11 + n_d).permutation(n)[:n_d]
        resid = np.zeros(n, np.float32)
        resid[chosen] = (0.25 * (1 + np.arange(n_d))).astype(np.float32)
        in_sd = np.zeros(n, bool)
        in_sd[chosen] = True
        other = np.flatnonzero(~in_sd)
        covered, meas = np.ones(n, bool), np.ones(n, bool)
        covered[other[::2]] = False
        meas[other[1::2]] = False
        x = crafted_inputs(H, W, resid, covered=covered, meas=meas)
        rng, wgt, vals, _ = _check_mask(gpu, x, 1.5, 0.0, tag=f"crafted n_d={n_d} {W}x{H}")
        assert vals[7] == n_d and vals[5] == [0.0, 0.25, 0.25][n_d] and vals[0] == meas.sum()
        assert vals[2] == [0, 0, 1][n_d]  # of {0.25, 0.5} the gate at 1.5 x 0.25 removes 0.5
        assert np.all(rng.reshape(-1)[~covered & meas] == 1)  # uncovered: new surface, kept


# -------------------------------------------------------------------------------------------------- 2. the weighted loss
# the shapes of test_gpu_train.py::test_loss_matches_oracle with their reasons: the smallest image with an interior, odd
# sizes, the strip seams of the streaming kernel (52 rows x 482 flat columns: ragged last strip / column block, exactly one,
# one more than one), and with w = 0 the L1-only kernel at any size
LOSS_SHAPES = [(11, 11, 0.1), (37, 53, 0.1), (53, 483, 0.3), (105, 161, 0.1), (52, 160, 0.5), (104, 322, 0.2), (12, 700, 1.0),
               (40, 33, 0.0), (5, 7, 0.0)]
_LOSS = {}


def _loss_case(h, w):
    """(x, y) of test_loss_matches_oracle and the three weight maps of a shape, computed once, never modified."""
    if (h, w) not in _LOSS:
        rng = np.random.default_rng(h * 1000 + w)
        x = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
        y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1).astype(np.float32)
        y[::7, ::5] = x[::7, ::5]  # exact ties: sign(0) = 0
        # (b) a binary rectangle whose vertical edges cross the strip seam at row 52 and whose horizontal edges cross the column
        # seams (pixel 160 | 161, 321 | 322, 482 | 483, 642 | 643), wherever the image has them
        rect = np.zeros((h, w), np.float32)
        rect[h // 4:max(3 * h // 4, min(h, 56)), w // 4:max(3 * w // 4, min(w, 166))] = 1.0
        # (c) uniform in [0, 1] with a tenth exact zeros
        wr = np.random.default_rng(77 + h + w)
        flt = wr.uniform(0, 1, (h, w)).astype(np.float32)
        flt[wr.uniform(size=(h, w)) < 0.10] = 0.0
        _LOSS[(h, w)] = (x, y, rect, flt)
    return _LOSS[(h, w)]


def _weighted(gpu, h, w, sw, x, y, m, sums=None):
    """Two calls into a NaN-filled gradient -> (grad, values) in numpy; asserts the runs are bitwise equal."""
    from gs_train import WeightedImageLoss

    loss = WeightedImageLoss(h, w, sw, gpu)
    tx, ty, tm = (torch.from_numpy(a).to(gpu) for a in (x, y, m))
    s = weight_sums(m) if sums is None else sums
    out = []
    for _ in range(2):
        loss.grad.fill_(float("nan"))
        loss.values.fill_(float("nan"))
        g = loss(tx, ty, tm, *s)
        assert g is loss.grad
        out.append((g.clone(), loss.values.clone()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and torch.equal(out[0][1], out[1][1])
    return out[0][0].cpu().numpy(), out[0][1].cpu().numpy()


def _far_from_weight(m):
    """Pixels of weight zero that lie further than 5 (rows or columns) from every interior pixel of non-zero weight."""
    h, w = m.shape
    src = (m > 0) & interior(h, w)
    near = np.zeros((h, w), bool)
    pad = np.pad(src, 5)
    for dy in range(11):
        for dx in range(11):
            near |= pad[dy:dy + h, dx:dx + w]
    return (m == 0) & ~near


@pytest.mark.parametrize("h,w,sw", LOSS_SHAPES)
def test_all_ones_weights_give_the_unweighted_loss_bit_for_bit(gpu, h, w, sw):
    """(a) Multiplying by 1.0f is exact and the operation order is the unweighted kernel's."""
    from gs_train import ImageLoss, weight_sums as device_sums

    x, y, _, _ = _loss_case(h, w)
    ones = np.ones((h, w), np.float32)
    assert device_sums(torch.from_numpy(ones).to(gpu)) == weight_sums(ones) == \
        (float(h * w), float((h - 10) * (w - 10)) if h > 10 and w > 10 else 0.0)
    g, vals = _weighted(gpu, h, w, sw, x, y, ones)
    plain = ImageLoss(h, w, sw, gpu)
    pg = plain(torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)).cpu().numpy()
    assert np.array_equal(_bits(g), _bits(pg)) and np.array_equal(_bits(vals), _bits(plain.values.cpu().numpy()))
    assert np.abs(g).max() > 0


@pytest.mark.parametrize("kind", ["rectangle", "float"])
@pytest.mark.parametrize("h,w,sw", LOSS_SHAPES)
def test_weighted_loss_matches_the_float64_helper(gpu, h, w, sw, kind):
    """(b) the binary rectangle, (c) float weights: values within 1e-6 / 2e-6 / 2e-6 (l1, ssim, loss -- the terms remain weighted
    means of quantities in [0, 1]) and the gradient within 2e-5 of its largest entry, the bounds of test_loss_matches_oracle;
    exact zeros where the weight is zero and no weighted interior pixel is within reach."""
    x, y, rect, flt = _loss_case(h, w)
    m = rect if kind == "rectangle" else flt
    g, vals = _weighted(gpu, h, w, sw, x, y, m)
    lo, l1, ssim, grad = weighted_l1_ssim_loss(x, y, m, sw)
    err = np.abs(g - grad).max()
    print(f"weighted loss {w}x{h} w={sw} {kind}: values {vals.tolist()} vs ({lo}, {l1}, {ssim}); gradient error {err:.3e} of "
          f"{np.abs(grad).max():.3e}")
    assert abs(vals[1] - l1) < 1e-6 and abs(vals[2] - ssim) < 2e-6 and abs(vals[0] - lo) < 2e-6
    assert err < 2e-5 * np.abs(grad).max(), (err, np.abs(grad).max())
    far = _far_from_weight(m) if sw > 0 else (m == 0)
    assert far.any() or kind == "float" or (h, w) == (11, 11)  # (11 x 11: its one interior pixel reaches every pixel)
    assert not _bits(g[far]).any()  # exactly +0.0
    assert np.abs(g[m > 0]).max() > 0


@pytest.mark.parametrize("h,w,sw", [s for s in LOSS_SHAPES if s[2] > 0])
def test_zero_interior_weights_leave_the_l1_term_alone(gpu, h, w, sw):
    """(d) Zero in the whole interior, one on the border: the SSIM value and its part of the gradient are exactly zero -- the
    gradient is a m sign(x - y) with a = (float)((1 - w) / (3 weight_sum)), bit for bit -- and the L1 value matches."""
    x, y, _, _ = _loss_case(h, w)
    m = np.ones((h, w), np.float32)
    m[5:h - 5, 5:w - 5] = 0.0
    s = weight_sums(m)
    assert s[1] == 0.0 and s[0] == h * w - (h - 10) * (w - 10)
    g, vals = _weighted(gpu, h, w, sw, x, y, m)
    lo, l1, ssim, _ = weighted_l1_ssim_loss(x, y, m, sw)
    a = np.float32((1.0 - float(np.float32(sw))) / (3.0 * s[0]))
    want = (a * np.sign(x - y) * m[:, :, None]).astype(np.float32)
    want[m == 0] = 0.0  # (+0.0 under a zero weight, whatever the sign)
    assert np.array_equal(_bits(g), _bits(want))
    assert vals[2] == 0.0 and ssim == 0.0 and abs(vals[1] - l1) < 1e-6 and abs(vals[0] - lo) < 2e-6
    assert abs(vals[0] - (1.0 - sw) * l1) < 2e-6  # no SSIM term in the loss either


@pytest.mark.parametrize("h,w,sw", LOSS_SHAPES)
def test_all_zero_weights_give_exact_zeros(gpu, h, w, sw):
    """(e) Both sums 0: the gradient is exactly zero everywhere and the values are (0, 0, 0)."""
    x, y, _, _ = _loss_case(h, w)
    g, vals = _weighted(gpu, h, w, sw, x, y, np.zeros((h, w), np.float32), sums=(0.0, 0.0))
    assert not _bits(g).any() and not _bits(vals).any()


# ------------------------------------------------------------------------------------------------ 3. the occluder keyframe
_OCC = {}


def _occluder(gpu):
    """The occluder frame of test_gpu_track_gate.py at its true pose, the clean frame, the map rendered there with its aux
    maps, and the GateMask of TrackOptions(depth_gate_k=10) on them.  Built once."""
    if not _OCC:
        from gs_frame import FrameRenderer
        from gs_track import TrackOptions
        from gs_train import GateMask
        from test_gpu_track_gate import OCC_COLS, OCC_ROWS, _frame

        params, cam, _, _, img, rng = _frame(gpu, occluded=True)
        _, _, _, _, clean_img, clean_rng = _frame(gpu, occluded=False)
        r = FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False)
        rimg, _, D, A = r.forward(*params, cam, training=False, aux=True)
        rimg, D, A = rimg.contiguous().clone(), D.contiguous().clone(), A.contiguous().clone()
        gm = GateMask.from_track_options(img.shape[0], img.shape[1], TrackOptions(depth_gate_k=10.0), gpu)
        gm(rimg, D, A, img, rng)
        occ = torch.zeros(img.shape[:2], dtype=torch.bool, device=gpu)
        occ[OCC_ROWS, OCC_COLS] = True
        _OCC.update(params=params, cam=cam, img=img, rng=rng, clean_img=clean_img, clean_rng=clean_rng, D=D, A=A, gm=gm, occ=occ)
    return _OCC


def test_the_gate_removes_the_occluder_from_a_keyframe(gpu):
    """At least 99 % of the 5,760 occluder pixels lose their range and have weight 0, at most 1 % of the 13,440 others do
    (profiles/track_gate.txt: 5,760 and 15 at a pose 1e-6 off); seeding then selects at least 5,000 pixels from the raw range
    and at most 1 % of that from the gated one."""
    from gs_seed import seed_from_depth

    o = _occluder(gpu)
    gm, occ, rng = o["gm"], o["occ"], o["rng"]
    assert int(occ.sum()) == 5760 and occ.numel() - 5760 == 13440
    lost_range, lost_weight = (gm.range == 0) & (rng > 0), gm.weight == 0
    in_occ, outside = int((lost_range & lost_weight & occ).sum()), int(((lost_range | lost_weight) & ~occ).sum())
    vals = gm.values.tolist()
    print(f"occluder keyframe: {in_occ} of 5760 occluder pixels lose range and weight, {outside} of the 13440 others lose "
          f"either; values {vals}")
    assert in_occ >= 0.99 * 5760
    assert outside <= 0.01 * 13440
    assert vals[2] == int(lost_range.sum()) and vals[3] == int((gm.weight != 0).sum())
    raw = int(seed_from_depth(o["img"], rng, o["cam"], rendered=(o["D"], o["A"]))[0].shape[0])
    gated = int(seed_from_depth(o["img"], gm.range, o["cam"], rendered=(o["D"], o["A"]))[0].shape[0])
    print(f"  seeding selects {raw} pixels from the raw range, {gated} from the gated one")
    assert raw >= 5000 and gated <= 0.01 * raw


def test_a_map_does_not_absorb_what_its_tracker_rejected(gpu):
    """Three Trainers on copies of the map, one view each, the same 30 steps (gs_slam's mapping options): (A) the occluded
    target with the raw range, (B) the occluded target with the gated range and weight, (C) the clean frame.  The unweighted
    colour loss of the view against the CLEAN target afterwards: the gated fit is better than the ungated one and sits nearer
    the clean fit than the ungated one."""
    from gs_frame import FrameRenderer
    from gs_slam import _map_train_options
    from gs_train import ImageLoss, Trainer

    o = _occluder(gpu)
    gm, cam = o["gm"], o["cam"]
    H, W = o["img"].shape[:2]
    opt = _map_train_options()
    legs = {"A": (o["img"], o["rng"], None), "B": (o["img"], gm.range.clone(), gm.weight.clone()),
            "C": (o["clean_img"], o["clean_rng"], None)}
    out = {}
    for name, (img, rng, wgt) in legs.items():
        tr = Trainer([p.detach().clone() for p in o["params"]], [cam], [img], opt, max_pairs=1 << 21, depths=[rng],
                     weights=None if wgt is None else [wgt])
        assert (tr.weights is None) == (wgt is None)
        for i in range(30):
            tr.train_step(i, 0)
        r = FrameRenderer(gpu, max_pairs=1 << 21, training=False, auto_grow=True)
        image = r.forward(*tr.flat.params, cam, training=False)[0].contiguous()
        probe = ImageLoss(H, W, opt.ssim_weight, gpu)
        probe(image, o["clean_img"])
        out[name] = float(probe.values[0])
    print(f"colour loss against the clean target after 30 steps: L_A (ungated) {out['A']:.6f}, L_B (gated) {out['B']:.6f}, "
          f"L_C (clean) {out['C']:.6f}")
    assert out["B"] < out["A"]
    assert abs(out["B"] - out["C"]) < abs(out["A"] - out["B"])
