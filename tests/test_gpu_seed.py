"""GPU tier of seeding from RGB-D frames (csrc/seed.hip through gs_seed / gs_train.Trainer.seed_from_view).

The reference has no counterpart of this step: the selected set is held against the float32 restatement of the decision
(tests/seed_ref.py: exactly, order included), what a pixel becomes against float64 closed forms within bounds counted from
the kernel's fp32 operations, the whole against the renderer (a seeded surface renders closed and at its depth, and is not
seeded twice), and the Trainer hook against a fit that lacks it."""
import math

import numpy as np
import pytest
import torch

from gs_colmap import initialize_sh
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_seed import DEFAULTS, seed_apply, seed_classify, seed_from_depth, seed_options
from gs_testutil import general_rotation, to_torch
from gs_train import ImageLoss, TrainOptions, Trainer
from seed_ref import gaussians, lattice, select

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24  # one fp32 rounding, relative


def _camera(W, H, yaw=17.0, tran=(0.4, -0.3, 0.8), general=False):
    cam = make_camera(W, H, yaw_deg=yaw)
    if general:  # gs_testutil.general_camera's rotation: no entry of rot zero, one, or equal in magnitude to another
        cam.rot = general_rotation(35.0, -12.0, 10.0)
    cam.focal_y = 0.8 * W  # fx != fy
    cam.tran = np.asarray(tran, np.float32)
    return cam


def _inputs(H, W, seed):
    """As tests/test_gpu_rgbd.py::_loss_inputs: A and D straddle both criteria (alpha_thresh 0.5; D / (A z) in [0.7, 1.3] around
    1 / (1 - front_rel)), ~30 % of the target without a measurement, of all four kinds; colours include exact 0 and 1."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.02, 1.0, (H, W)).astype(np.float32)
    z = rng.uniform(0.3, 12.0, (H, W)).astype(np.float32)
    D = (A * z * rng.uniform(0.7, 1.3, (H, W))).astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.30
    kind = rng.integers(0, 4, (H, W))
    z[bad & (kind == 0)] = 0.0
    z[bad & (kind == 1)] = -z[bad & (kind == 1)]
    z[bad & (kind == 2)] = np.inf
    z[bad & (kind == 3)] = np.nan
    img = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    edge = rng.uniform(size=(H, W, 3))
    img[edge < 0.02] = 0.0
    img[edge > 0.98] = 1.0
    return D, A, z, img


def _activated(scale, act):
    s = scale.astype(np.float64)
    return np.abs(s) + float(np.float32(1e-4)) if act == "abs" else np.exp(s)


# ------------------------------------------------------------------------------------- 1. kernel against the restatement
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("H,W", [(48, 64), (187, 250), (1080, 1920)])
def test_seed_matches_the_restatement(gpu, H, W, stride):
    """Selected set, order and counts: exactly the float32 restatement's.  Values against float64 closed forms, every bound a
    count of the kernel's fp32 roundings (each <= 2^-24 relative):
      pos    <= 32 x 2^-24 x (range + |tran|) per coordinate: a camera-space coordinate carries at most 9 roundings (u or v: 1;
                u u, v v, two sums, the root, z / root: 6 on z_cam, none of them amplified; the product; minus tran), the three
                of them meet in rot^T (entries <= 1 in magnitude) with 3 products and 2 sums more: 27 + 5.  1.9e-6.
      scale  activated value <= 12 x 2^-24 x sigma: z_cam as above with u, v (7), scale_factor x stride, x z_cam, (fx + fy), the
                division, the subtraction of 1e-4 (abs) -- or, exp, the stored log within 12 x 2^-24 + 4 x 2^-24 |log sigma|
                (logf: 2 ulp).
      opa    one rounding of the double-precision logit.
      colour logits <= (2 + 4 |logit|) x 2^-24: 1 - c and the quotient (the logarithm turns their relative error into an absolute
                one), logf within 2 ulp of its result.
    quat exact.  Measured maxima on an MI355X, as shares of the bounds: profiles/seed_rgbd.txt."""
    _check_seed_matches_the_restatement(gpu, H, W, stride, _camera(W, H))


def test_seed_matches_the_restatement_under_a_general_rotation(gpu):
    """The same statement at 187 x 250, stride 2, with a rotation about no single axis: under test_seed_matches_the_restatement's
    yaw-only matrix (four exact zeros, an exact one) rot^T and rot give the same y row, and a kernel that reads one entry of
    rot for another can place every Gaussian where it belongs."""
    _check_seed_matches_the_restatement(gpu, 187, 250, 2, _camera(250, 187, general=True))


def _check_seed_matches_the_restatement(gpu, H, W, stride, cam):
    D, A, z, img = _inputs(H, W, seed=H + W + stride)
    at, fr, sf, p0 = 0.5, 0.1, 0.7, 0.9
    sel, meas = select(z, D, A, stride, at, fr)
    n_sel, n_meas = int(sel.sum()), int(meas.sum())
    assert 0.1 * n_meas < n_sel < 0.9 * n_meas  # the inputs exercise both outcomes (checked on the CPU)
    assert (meas & (A < at)).any() and (meas & ~(A < at) & sel).any()  # ... and both criteria
    tD, tA, tz, timg = (torch.from_numpy(x).to(gpu) for x in (D, A, z, img))
    for act in ("abs", "exp") if stride == 2 else ("abs",):
        opts = seed_options(stride, at, fr, sf, p0, 3, act)
        counts, _ = seed_classify(tz, (tD, tA), opts)
        assert counts.tolist() == [n_sel, n_meas]
        pos, quat, scale, opa, rgb = (t.cpu().numpy() for t in seed_from_depth(
            timg, tz, cam, rendered=(tD, tA), stride=stride, alpha_thresh=at, front_rel=fr, scale_factor=sf, opa_init=p0,
            scale_activation=act))
        assert pos.shape == (n_sel, 3) and rgb.shape == (n_sel, 3)
        ref = gaussians(img, z, cam, sel, stride, sf, p0)
        # the order: a Gaussian projects back onto the centre of ITS pixel, row-major
        p_c = pos.astype(np.float64) @ np.asarray(cam.rot, np.float64).T + np.asarray(cam.tran, np.float64)
        px = p_c[:, 0] / p_c[:, 2] * float(np.float32(cam.focal_x)) + (-(-W // 16) * 16) / 2 - 0.5 - ((-(-W // 16) * 16) - W) // 2
        py = p_c[:, 1] / p_c[:, 2] * float(np.float32(cam.focal_y)) + (-(-H // 16) * 16) / 2 - 0.5 - ((-(-H // 16) * 16) - H) // 2
        assert np.array_equal(np.rint(px).astype(np.int64), ref["xs"]) and np.array_equal(np.rint(py).astype(np.int64), ref["ys"])
        assert max(np.abs(px - ref["xs"]).max(), np.abs(py - ref["ys"]).max()) < 0.05
        e_pos = (np.abs(pos - ref["pos"]).max(axis=1) / ref["reach"]).max() / EPS
        sig = ref["sigma"]
        assert np.array_equal(scale[:, 0], scale[:, 1]) and np.array_equal(scale[:, 0], scale[:, 2])
        if act == "abs":
            e_scale = (np.abs(_activated(scale[:, 0], act) - sig) / sig).max() / EPS
            b_scale = 12.0
        else:
            e_scale = (np.abs(scale[:, 0] - np.log(sig)) / (12.0 + 4.0 * np.abs(np.log(sig)))).max() / EPS
            b_scale = 1.0
        e_opa = np.abs(opa - ref["opa"]).max() / abs(ref["opa"]) / EPS
        e_rgb = (np.abs(rgb - ref["logit"]) / (2.0 + 4.0 * np.abs(ref["logit"]))).max() / EPS
        print(f"seed {H}x{W} stride {stride} {act}: selected {n_sel} of {n_meas} measured; max error in roundings (2^-24): "
              f"pos {e_pos:.2f} of 32 (x reach), scale {e_scale:.2f} of {b_scale:g}, opa {e_opa:.2f} of 1, "
              f"colour {e_rgb:.3f} of 1 (x (2 + 4 |logit|))")
        assert e_pos <= 32.0 and e_scale <= b_scale and e_opa <= 1.0 and e_rgb <= 1.0
        assert np.array_equal(quat, np.tile(np.array([1, 0, 0, 0], np.float32), (n_sel, 1)))
        assert np.array_equal(opa, np.full(n_sel, opa[0], np.float32)) and np.isfinite(rgb).all()
        assert np.abs(rgb).max() <= math.log(511.0) * (1 + 4 * EPS)  # the clamp: 1 / 512 from 0 and from 1
    # no maps: every measured lattice pixel
    out = seed_from_depth(timg, tz, cam, stride=stride, alpha_thresh=at, front_rel=fr, scale_factor=sf, opa_init=p0)
    ys, xs = lattice(H, W, stride)
    assert out[0].shape[0] == n_meas == int((np.isfinite(z[ys, xs]) & (z[ys, xs] > 0)).sum())
    ref_all = gaussians(img, z, cam, meas, stride, sf, p0)
    assert (np.abs(out[0].cpu().numpy() - ref_all["pos"]).max(axis=1) / ref_all["reach"]).max() <= 32 * EPS


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("color_dim", [27, 48])
def test_seed_sh_rows_carry_the_dc_of_initialize_sh(gpu, color_dim, stride):
    """color_dim 27 / 48: the DC coefficient of each channel is gs_colmap.initialize_sh's of the rgb logits (the same fp32
    division), every other coefficient exactly zero, everything else as for rgb -- bit for bit."""
    H, W = 187, 250
    D, A, z, img = _inputs(H, W, seed=7 + stride)
    cam = _camera(W, H)
    tD, tA, tz, timg = (torch.from_numpy(x).to(gpu) for x in (D, A, z, img))
    kw = dict(rendered=(tD, tA), stride=stride, alpha_thresh=0.5, front_rel=0.1)
    base = [t.cpu().numpy() for t in seed_from_depth(timg, tz, cam, **kw)]
    got = [t.cpu().numpy() for t in seed_from_depth(timg, tz, cam, color_dim=color_dim, **kw)]
    n, nb = base[0].shape[0], color_dim // 3
    assert n > 1000 and got[4].shape == (n, color_dim)
    for a, b in zip(base[:4], got[:4]):
        assert np.array_equal(a, b)
    sh = got[4].reshape(n, 3, nb)
    assert np.array_equal(sh[:, :, 0], initialize_sh(base[4]).reshape(n, 3, 9)[:, :, 0])
    assert not sh[:, :, 1:].any()
    if color_dim == 27:
        assert np.array_equal(got[4], initialize_sh(base[4]))


# ------------------------------------------------------------------------------------------ 2. repeatability and capacity
@pytest.mark.parametrize("H,W,stride,color_dim", [(187, 250, 2, 3), (187, 250, 1, 27), (1080, 1920, 1, 3), (1080, 1920, 3, 48)])
def test_seed_is_bitwise_repeatable_and_respects_offset_and_capacity(gpu, H, W, stride, color_dim):
    D, A, z, img = _inputs(H, W, seed=99)
    cam = _camera(W, H)
    tD, tA, tz, timg = (torch.from_numpy(x).to(gpu) for x in (D, A, z, img))
    opts = seed_options(stride, 0.5, 0.1, color_dim=color_dim)
    counts, ws = seed_classify(tz, (tD, tA), opts)
    n = int(counts[0])
    assert n == int(select(z, D, A, stride, 0.5, 0.1)[0].sum()) > 0
    offset, tail = 5, 11
    cap = offset + n + tail
    shapes = [(cap, 3), (cap, 4), (cap, 3), (cap,), (cap, color_dim)]

    def garbage(seed):
        g = torch.Generator(gpu).manual_seed(seed)
        return [torch.randn(s, device=gpu, generator=g) * 100 for s in shapes]

    runs = []
    for seed in (1, 2):
        out = garbage(seed)
        before = [t.clone() for t in out]
        c2, w2 = seed_classify(tz, (tD, tA), opts)
        seed_apply(timg, tz, cam, opts, out, offset, c2, w2)
        for t, b in zip(out, before):  # rows outside [offset, offset + n) are untouched
            assert torch.equal(t[:offset], b[:offset]) and torch.equal(t[offset + n:], b[offset + n:])
            assert not torch.equal(t[offset:offset + n], b[offset:offset + n])
        runs.append([t[offset:offset + n].clone() for t in out])
    for a, b in zip(*runs):
        assert torch.equal(a, b)  # bit for bit, whatever the buffers held
    # one row short: nothing is written, the count still reports the need
    out = garbage(3)
    before = [t.clone() for t in out]
    seed_apply(timg, tz, cam, opts, out, offset, counts, ws, capacity=offset + n - 1)
    for t, b in zip(out, before):
        assert torch.equal(t, b)
    assert int(counts[0]) == n
    seed_apply(timg, tz, cam, opts, out, offset, counts, ws, capacity=offset + n)  # ... and exactly enough is enough
    for t, r, b in zip(out, runs[0], before):
        assert torch.equal(t[offset:offset + n], r) and torch.equal(t[offset + n:], b[offset + n:])


# ---------------------------------------------------------------------------------------- 3. round trip through the renderer
def _plane_view(W, H, normal, dist):
    """Range map of the plane n . p_c = dist (camera space) along the renderer's pixel rays, and a procedural colour image."""
    from seed_ref import pixel_rays

    cam = _camera(W, H, yaw=9.0, tran=(0.2, -0.1, 0.3))
    cam.focal_y = cam.focal_x
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = pixel_rays(cam, ys, xs)
    n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    norm = np.sqrt(u * u + v * v + 1.0)
    z_cam = dist / (n[0] * u + n[1] * v + n[2])
    rng = (z_cam * norm).astype(np.float32)
    img = np.stack([0.5 + 0.4 * np.sin(xs / 7.0) * np.cos(ys / 5.0), 0.5 + 0.4 * np.cos(xs / 11.0 + ys / 13.0),
                    0.2 + 0.6 * ((xs // 8 + ys // 8) % 2)], 2).astype(np.float32)
    return cam, rng, img, z_cam


@pytest.mark.parametrize("name,normal,dist", [("fronto-parallel", (0.0, 0.0, 1.0), 2.0), ("tilted", (0.3, -0.2, 1.0), 2.5)])
def test_seeded_plane_renders_closed_and_is_not_seeded_twice(gpu, name, normal, dist):
    """A plane beyond `near`, seeded into an empty model at stride 1 with the defaults and rendered from the same camera.
      A >= opa_init (1 - 4e-6) at every pixel: a pixel's own Gaussian sits on its centre up to the fp32 error of two projections
        (<= 2e-3 pixel: 32 roundings of 2^-24 on coordinates of ~3 units at ~60 pixels per unit, twice, and the pixel grid's own),
        so its exponent there is <= (2e-3)^2 / (2 x 0.7^2) = 4e-6, and A = 1 - prod (1 - alpha_i) >= alpha_own.
      D / A lies between the smallest and the largest range of the plane over the 13 x 13 pixels around the pixel, widened by
        1e-5 of the range: D / A is a weighted mean of the ranges of the Gaussians the pixel composites, all of them ON the plane;
        sigma is 0.7 pixel (x (1 + u^2 + v^2) <= 1.5 off the axis), a Gaussian is listed for the tiles its 2.45 sigma box meets,
        and whatever a pixel composites from beyond 6 pixels weighs < exp(-(6 / 1.05)^2 / 2) = 1e-7 of the mean.
      A second seeding from that view with the rendered maps selects nothing.
      The degree-2 SH set renders the same image as the rgb set within the frame path's image tolerance, 5e-5."""
    W, H = 160, 112
    cam, rng, img, z_cam = _plane_view(W, H, normal, dist)
    assert z_cam.min() > 2 * cam.near
    trng, timg = torch.from_numpy(rng).to(gpu), torch.from_numpy(img).to(gpu)
    params = seed_from_depth(timg, trng, cam)
    assert params[0].shape[0] == H * W
    r = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=True)
    image, depth, alpha = (t.clone() for t in r.render_aux(*params, cam))
    a, e = alpha.cpu().numpy().astype(np.float64), (depth / alpha).cpu().numpy().astype(np.float64)
    print(f"{name} plane: alpha min {a.min():.6f} (opa_init {DEFAULTS['opa_init']}), |D/A - range| max "
          f"{np.abs(e - rng).max():.3e} (range {rng.min():.3f} .. {rng.max():.3f})")
    assert a.min() >= float(np.float32(DEFAULTS["opa_init"])) * (1 - 4e-6)
    R = 6
    pad = np.pad(rng.astype(np.float64), R, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(pad, (2 * R + 1, 2 * R + 1))
    lo, hi = win.min(axis=(2, 3)), win.max(axis=(2, 3))
    assert (e >= lo * (1 - 1e-5)).all() and (e <= hi * (1 + 1e-5)).all()
    again = seed_from_depth(timg, trng, cam, rendered=(depth, alpha))
    assert again[0].shape[0] == 0
    same = seed_from_depth(timg, trng, cam, rendered=(depth, alpha), append_to=params)
    assert all(x is y for x, y in zip(same, params))
    sh = seed_from_depth(timg, trng, cam, color_dim=27)
    image_sh = r.render_aux(*sh, cam)[0]
    err = float((image_sh - image).abs().max())
    print(f"{name} plane: SH-seeded against rgb-seeded image: max |diff| {err:.2e}; image against the colour frame: mean |diff| "
          f"{float((image - timg).abs().mean()):.4f}")
    assert err <= 5e-5
    # z-depth in, the same Gaussians out: both sets within the kernel's 32 roundings of the truth, the range maps two apart
    z_kind = seed_from_depth(timg, torch.from_numpy(z_cam.astype(np.float32)).to(gpu), cam, depth_kind="z")
    assert float((z_kind[0] - params[0]).abs().max()) <= 66 * EPS * float(rng.max() + np.linalg.norm(cam.tran))


def test_append_keeps_the_old_rows_bit_for_bit(gpu):
    W, H = 160, 112
    cam, rng, img, _ = _plane_view(W, H, (0.0, 0.0, 1.0), 2.0)
    trng, timg = torch.from_numpy(rng).to(gpu), torch.from_numpy(img).to(gpu)
    old = to_torch(make_scene(777, W, H, seed=4), gpu)
    new = seed_from_depth(timg, trng, cam, stride=4)
    both = seed_from_depth(timg, trng, cam, stride=4, append_to=old)
    for o, n, b in zip(old, new, both):
        assert torch.equal(b[:777], o) and torch.equal(b[777:], n)
    with pytest.raises(RuntimeError):
        seed_from_depth(timg, trng, cam, color_dim=27, append_to=old)


# ------------------------------------------------------------------------------------------------------------ 4. Trainer
def _views(gpu, W, H):
    """Truth: a small make_scene; colour targets rendered from it, range targets D / A where A >= 0.9 (0 elsewhere); three views
    that overlap only partly (yaw -16, 0, +16 degrees of a 67-degree field of view, and a sideways step)."""
    scene = make_scene(6_000, W, H, seed=31)
    cams = []
    for yaw, tx in ((0.0, 0.0), (-16.0, -0.5), (16.0, 0.5)):
        c = make_camera(W, H, yaw_deg=yaw)
        c.tran = np.array([tx, 0.0, 0.0], np.float32)
        cams.append(c)
    gt = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=True)
    images, ranges = [], []
    for cam in cams:
        img, _, d, a = r.forward(*gt, cam, training=False, aux=True)
        images.append(img.clamp(0, 1).clone())
        ranges.append(torch.where(a >= 0.9, d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous())
    return cams, images, ranges


def _trainer(start, cams, images, ranges, steps, **kw):
    opt = TrainOptions(n_iters=steps + 1, n_iters_warmup=5, depth_weight=0.2)
    return Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 21, depths=ranges, **kw)


def test_trainer_seed_from_view_extends_the_set_once(gpu):
    W, H = 160, 112
    cams, images, ranges = _views(gpu, W, H)
    start = seed_from_depth(images[0], ranges[0], cams[0])
    for kw in ({}, {"per_view_stat": True, "densify": True}, {"densify": True}):
        tr = _trainer(start, cams, images, ranges, 50, **kw)
        for i in range(4):
            tr.train_step(i, 0)
        n0, added = tr.n_gaussians, []
        for v in (1, 2):
            flat_before = tr.flat
            k = tr.seed_from_view(v, 4)
            assert k > 0 and tr.n_gaussians == n0 + sum(added) + k and tr.flat is not flat_before
            added.append(k)
            flat, p, m = tr.flat, tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone()
            assert tr.seed_from_view(v, 4) == 0  # the view is explained now
            assert tr.flat is flat and torch.equal(tr.flat.flat_param, p) and torch.equal(tr.optimizer.exp_avg, m)
        for i in range(4, 10):
            tr.train_step(i, i % 3)
        # after steps have moved the optimizer state, a call that selects nothing still leaves it alone
        p, m, v2 = tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone()
        again = tr.seed_from_view(0, 10, alpha_thresh=-1.0, front_rel=0.999)  # nothing can be selected with these
        assert again == 0 and torch.equal(tr.flat.flat_param, p) and torch.equal(tr.optimizer.exp_avg, m)
        assert torch.equal(tr.optimizer.exp_avg_sq, v2)
        kw_name = "default" if not kw else ",".join(f"{a}={b}" for a, b in kw.items())
        print(f"seed_from_view [{kw_name}]: {n0} Gaussians from view 0, + {added[0]} from view 1, + {added[1]} from view 2")
        if kw.get("per_view_stat"):
            split = (added, tr.flat.flat_param.clone())
        elif kw.get("densify"):
            assert added == split[0] and torch.equal(tr.flat.flat_param, split[1])  # per_view_stat=True: the default's result
    with pytest.raises(RuntimeError):
        _trainer(start, cams, images, [ranges[0], None, ranges[2]], 50).seed_from_view(1, 0)
    with pytest.raises(RuntimeError):
        Trainer([t.clone() for t in start], cams, images, TrainOptions()).seed_from_view(1, 0)


def test_seeding_the_new_views_helps_the_fit(gpu):
    """From seed_from_depth(view 0) alone, 90 depth-supervised steps over the three views in a fixed order, with and without
    seed_from_view(1), seed_from_view(2) in front of them.  On views 1 and 2 (mean of the two) the seeded run must end with a
    strictly lower colour loss ((1 - w) L1 + w (1 - SSIM), w = 0.1) and a strictly lower depth term (mean |D - A z| over the
    measured pixels).  The run WITHOUT seeding is the baseline.  Measured on an MI355X: profiles/seed_rgbd.txt."""
    W, H = 160, 112
    cams, images, ranges = _views(gpu, W, H)
    start = seed_from_depth(images[0], ranges[0], cams[0])
    steps = 90
    order = np.random.default_rng(5).integers(0, 3, steps)

    def evaluate(tr):
        r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=True)
        colour, depth = [], []
        for v in (1, 2):
            img, _, d, a = r.forward(*tr.flat.params, cams[v], training=False, aux=True)
            probe = ImageLoss(H, W, tr.opt.ssim_weight, gpu)
            probe(img.contiguous(), images[v])
            colour.append(float(probe.values[0]))
            ok = ranges[v] > 0
            depth.append(float((d - a * ranges[v]).abs()[ok].mean()))
        return float(np.mean(colour)), float(np.mean(depth))

    def fit(seed_views):
        tr = _trainer(start, cams, images, ranges, steps)
        added = [tr.seed_from_view(v, 0) for v in seed_views]
        at_start = evaluate(tr)
        for i in range(steps):
            tr.train_step(i, int(order[i]))
        return at_start, evaluate(tr), tr.n_gaussians, added

    plain0, plain, n_plain, _ = fit(())
    seeded0, seeded, n_seeded, added = fit((1, 2))
    print(f"views 1 and 2, (colour loss, depth term): without seeding {plain0[0]:.4f}, {plain0[1]:.4f} -> {plain[0]:.4f}, "
          f"{plain[1]:.4f} ({n_plain} Gaussians); with seed_from_view {seeded0[0]:.4f}, {seeded0[1]:.4f} -> {seeded[0]:.4f}, "
          f"{seeded[1]:.4f} ({n_seeded} Gaussians, + {added})")
    assert all(k > 0 for k in added) and n_seeded == n_plain + sum(added)
    assert all(math.isfinite(x) for x in plain + seeded)
    assert seeded[0] < plain[0]
    assert seeded[1] < plain[1]
