"""GPU tier of the median-gated tracking loss (gs_loss_track_gated, gs_train.GatedTrackLoss) and of the Tracker with the gate
on: the device selection against np.sort of the kernel's own residual maps and the masks they imply, exactly; the gradients
inside the masks bit for bit against gs_loss_track; crafted sets for every level of the select; the gate off against the old
kernel; a frame with an occluder tracked with and without the gate.  include/gs_abi.h states the contract."""
import numpy as np
import pytest
import torch

from gs_track import TrackOptions, Tracker
from gs_train import GatedTrackLoss, TrackLoss
from test_gpu_track import H_, W_, _scene, _target
from track_gate_ref import crafted_inputs, gate_from_residuals, low_bits, powers_and_zeros
from track_ref import ALPHA_MIN, LOSS_CASES, loss_inputs, measured, perturbed_start, pose_errors

pytestmark = pytest.mark.gpu

CW, DW = 0.8, 1.3
_CACHE = {}


def _inputs(H, W, seed):
    """The numpy inputs of a size, computed once, never modified."""
    if (H, W) not in _CACHE:
        _CACHE[(H, W)] = loss_inputs(H, W, seed)
    return _CACHE[(H, W)]


def _run_gated(gl, t, scale, with_range=True):
    """One call into NaN-filled destinations -> clones of the three gradients, the eight values and the two residual maps."""
    for g in (gl.grad_image, gl.grad_depth, gl.grad_alpha, gl.resid_depth, gl.resid_color, gl.values):
        g.fill_(float("nan"))
    gi, gd, ga = gl(t[0], t[1], t[2], t[3], t[4] if with_range else None, scale)
    return [x.clone() for x in (gi, gd, ga, gl.values, gl.resid_depth, gl.resid_color)]


def _run_plain(H, W, t, scale, gpu, with_range=True):
    """gs_loss_track with the gate off, the same weights and scale -> (grad_image, grad_depth, grad_alpha, values) in numpy."""
    tl = TrackLoss(H, W, ALPHA_MIN, CW, DW, 0.0, gpu)
    out = tl(t[0], t[1], t[2], t[3], t[4] if with_range else None, scale)
    return [x.cpu().numpy() for x in out] + [tl.values.cpu().numpy()]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_contract(out, plain, x, k_d, k_c, floor_d, floor_c, couple, tag):
    """Everything the contract makes exact, from the kernel's own residual maps.  -> the reference dict."""
    I, D, A, T, z = x
    gi, gd, ga, vals, ra, rc = (o.cpu().numpy() for o in out)
    covered, meas = A >= np.float32(ALPHA_MIN), measured(z)
    ref = gate_from_residuals(ra, rc, covered, meas, k_d, k_c, floor_d, floor_c, couple)
    # the medians: the rank-(n - 1) // 2 element of the kernel's own residuals, by a sort
    sa, sc = np.sort(ra[~np.isnan(ra)]), np.sort(rc[~np.isnan(rc)])
    want_md = sa[(len(sa) - 1) // 2] if len(sa) else np.float32(0)
    want_mc = sc[(len(sc) - 1) // 2] if len(sc) else np.float32(0)
    print(f"{tag}: n_d {len(sa)} n_c {len(sc)} m_d {vals[5]!r} m_c {vals[6]!r} counted {vals[3]:.0f} / {vals[4]:.0f}")
    assert _bits(vals[5]) == _bits(want_md) and _bits(vals[6]) == _bits(want_mc), (vals[5], want_md, vals[6], want_mc)
    assert vals[7] == len(sa) == ref["n_d"]
    # the masks: inside, gs_loss_track's gradients bit for bit; outside, exact zeros; both counts exact
    pgi, pgd, pga = plain[:3]
    dm, cm = ref["dmask"], ref["cmask"]
    assert np.array_equal(_bits(gd)[dm], _bits(pgd)[dm]) and np.array_equal(_bits(ga)[dm], _bits(pga)[dm])
    assert np.array_equal(_bits(gi)[cm], _bits(pgi)[cm])
    assert not _bits(gd)[~dm].any() and not _bits(ga)[~dm].any() and not _bits(gi)[~cm].any()  # (+0.0, not -0.0)
    assert vals[3] == dm.sum() and vals[4] == cm.sum()
    return ref


# --------------------------------------------------------------------------------------------- 1. selection and masks
@pytest.mark.parametrize("couple", [True, False])
@pytest.mark.parametrize("H,W,seed", LOSS_CASES)
def test_selection_and_masks_are_exact(gpu, H, W, seed, couple):
    """k_d = k_c = 1.5, floors 0.  The exact checks of _check_contract on every pixel; each gate cuts 5 - 60 % of its set; the
    residual maps against fp64 (a within 1e-6 max(|D / A|, |z|) -- the two roundings of a quotient and a difference; measured
    6e-8 --, c within 1e-6, NaN exactly outside the sets); the three values within 1e-5 relative of an fp64 sum over the
    kernel's masks (the bound of test_track_loss_matches_fp64); two runs bitwise equal and everything written."""
    x = _inputs(H, W, seed)
    I, D, A, T, z = x
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    gl = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, 1.5, 1.5, 0.0, 0.0, couple, gpu, keep_residuals=True)
    out = _run_gated(gl, t, scale)
    out2 = _run_gated(gl, t, scale)
    for a, b in zip(out[:4], out2[:4]):
        assert torch.equal(a, b) and not torch.isnan(a).any()  # bitwise repeatable, everything written
    for a, b in zip(out[4:], out2[4:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # (the maps hold NaNs by contract)
    ref = _check_contract(out, _run_plain(H, W, t, scale, gpu), x, 1.5, 1.5, 0.0, 0.0, couple, f"gate {W}x{H} couple={couple}")
    # non-vacuity
    ra, rc = out[4].cpu().numpy(), out[5].cpu().numpy()
    with np.errstate(invalid="ignore"):
        cut_d = 1.0 - float((ra <= ref["t_d"]).sum()) / ref["n_d"]
        cut_c = 1.0 - float((rc <= ref["t_c"]).sum()) / ref["n_c"]
    print(f"  cut shares: depth {cut_d:.3f} colour {cut_c:.3f}")
    assert 0.05 <= cut_d <= 0.60 and 0.05 <= cut_c <= 0.60
    # the residual maps against fp64
    covered, meas = A >= np.float32(ALPHA_MIN), measured(z)
    s_d = covered & meas
    assert np.array_equal(np.isnan(ra), ~s_d) and np.array_equal(np.isnan(rc), ~covered)
    e64 = D.astype(np.float64)[s_d] / A.astype(np.float64)[s_d]
    z64 = z.astype(np.float64)[s_d]
    err_a = float((np.abs(ra[s_d] - np.abs(e64 - z64)) / np.maximum(np.abs(e64), np.abs(z64))).max())
    c64 = np.abs(I.astype(np.float64) - T.astype(np.float64)).sum(axis=2)
    err_c = float(np.abs(rc[covered] - c64[covered]).max())
    print(f"  residual maps vs fp64: a {err_a:.2e} (relative to max(|D/A|, |z|)), c {err_c:.2e}")
    assert err_a <= 1e-6 and err_c <= 1e-6
    # the values
    v = out[3].cpu().numpy().astype(np.float64)
    colour = scale * CW * float(c64[ref["cmask"]].sum())
    e_all = np.abs(D.astype(np.float64) / A.astype(np.float64) - np.where(meas, z, 0).astype(np.float64))
    depth = scale * DW * float(e_all[ref["dmask"]].sum())
    print(f"  values {v[:3].tolist()} vs fp64 {[colour + depth, colour, depth]}")
    for got, want in ((v[0], colour + depth), (v[1], colour), (v[2], depth)):
        assert want > 0 and abs(got - want) <= 1e-5 * want


# ---------------------------------------------------------------------------------------------------- 2. crafted sets
def _crafted_run(gpu, H, W, x, k_d, k_c=0.0, floor_d=0.0, couple=True, tag=""):
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    gl = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, k_d, k_c, floor_d, 0.0, couple, gpu, keep_residuals=True)
    out = _run_gated(gl, t, scale)
    ref = _check_contract(out, _run_plain(H, W, t, scale, gpu), x, k_d, k_c, floor_d, 0.0, couple, tag)
    return [o.cpu().numpy() for o in out], ref


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64), (1080, 1920)])
def test_crafted_every_residual_equal(gpu, H, W):
    """(a) D = 2: one bin holds every element at every level -- 2,073,600 of them at 1080p, beyond any 16-bit counter."""
    x = crafted_inputs(H, W, np.ones(H * W))
    (gi, gd, ga, vals, ra, rc), ref = _crafted_run(gpu, H, W, x, 1.5, tag=f"crafted equal {W}x{H}")
    assert vals[5] == 1.0 and vals[7] == H * W and vals[3] == H * W and vals[4] == H * W  # median 1, nothing cut
    assert np.all(ra == 1.0) and np.all(gd != 0)


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64)])
@pytest.mark.parametrize("kind", ["powers_and_zeros", "low_bits"])
def test_crafted_bit_pattern_order(gpu, H, W, kind):
    """(b) 2^-k, k = 1 .. 23, and exact zeros: the order of the bit patterns across exponents and the zero pattern.
    (c) 0.5 + j 2^-23: residuals the last level alone tells apart.  k_d = 1: the threshold is the median itself, so the
    gate keeps exactly the elements up to it."""
    resid = powers_and_zeros(H * W) if kind == "powers_and_zeros" else low_bits(H * W)
    x = crafted_inputs(H, W, resid)
    (gi, gd, ga, vals, ra, rc), ref = _crafted_run(gpu, H, W, x, 1.0, tag=f"crafted {kind} {W}x{H}")
    assert np.array_equal(ra.reshape(-1), resid)  # exact by construction
    m = np.sort(resid)[(H * W - 1) // 2]
    assert vals[5] == m and vals[3] == (resid <= m).sum() and 0 < vals[3] < H * W


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64)])
@pytest.mark.parametrize("n_d", [0, 1, 2, 10])
def test_crafted_small_sets(gpu, H, W, n_d):
    """(d) n_d = 0, 1, 2 and an even count, every other pixel unmeasured or uncovered: the lower median (of two elements the
    smaller; of ten the fifth), 0 for the empty set -- with which there is no depth term and coupling drops no colour."""
    n = H * W
    rng = np.random.default_rng(11 + n_d)
    chosen = rng.permutation(n)[:n_d]
    resid = np.zeros(n, np.float32)
    resid[chosen] = (0.25 * (1 + np.arange(n_d))).astype(np.float32)  # 0.25, 0.5, ...: distinct, exact
    in_sd = np.zeros(n, bool)
    in_sd[chosen] = True
    other = np.flatnonzero(~in_sd)
    covered, meas = np.ones(n, bool), np.ones(n, bool)
    covered[other[::2]] = False  # the others: alternately uncovered and unmeasured
    meas[other[1::2]] = False
    x = crafted_inputs(H, W, resid, covered=covered, meas=meas)
    (gi, gd, ga, vals, ra, rc), ref = _crafted_run(gpu, H, W, x, 1.5, tag=f"crafted n_d={n_d} {W}x{H}")
    assert vals[7] == n_d
    want = [0.0, 0.25, 0.25, 1.25][[0, 1, 2, 10].index(n_d)]
    assert vals[5] == want
    assert vals[3] == sum(1 for k in range(n_d) if 0.25 * (1 + k) <= 1.5 * want)
    if n_d == 0:
        assert vals[2] == 0.0 and not gd.any() and not ga.any() and vals[4] == covered.sum()  # colour: every covered pixel


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64)])
def test_crafted_median_zero_and_the_floor(gpu, H, W):
    """(e) more than half of the residuals are exact zeros: median 0, threshold 0 with floor 0 -- only the zeros count.
    (f) the same inputs with a floor of 0.3: the floor admits the residuals up to it."""
    n = H * W
    resid = np.where(np.arange(n) % 5 < 3, 0.0, np.where(np.arange(n) % 5 == 3, 0.25, 0.5)).astype(np.float32)
    np.random.default_rng(3).shuffle(resid)
    x = crafted_inputs(H, W, resid)
    (_, gd, _, vals, _, _), _ = _crafted_run(gpu, H, W, x, 1.5, tag=f"crafted median 0 {W}x{H}")
    assert vals[5] == 0.0 and vals[3] == (resid == 0).sum() and vals[2] == 0.0
    assert not gd.any()  # a zero residual has a zero gradient: sign(0) = 0
    (_, gd, _, vals, _, _), _ = _crafted_run(gpu, H, W, x, 1.5, floor_d=0.3, tag=f"crafted median 0, floor 0.3 {W}x{H}")
    assert vals[5] == 0.0 and vals[3] == (resid <= 0.25).sum() and vals[2] > 0.0
    assert np.array_equal(gd.reshape(-1) != 0, resid == 0.25)


@pytest.mark.parametrize("H,W", [(7, 9), (48, 64)])
def test_crafted_nan_and_inf_stay_outside(gpu, H, W):
    """(g) a NaN and an inf in D at covered, measured pixels with k_d > 0: outside S_d, not counted, zero gradients, NaN in
    the residual map, and the median is that of the others."""
    n = H * W
    resid = powers_and_zeros(n)
    I, D, A, T, z = crafted_inputs(H, W, resid)
    D = D.copy()
    D.reshape(-1)[5], D.reshape(-1)[n - 2] = np.nan, np.inf  # (n - 2: in the tail of 7 x 9)
    x = (I, D, A, T, z)
    (gi, gd, ga, vals, ra, rc), ref = _crafted_run(gpu, H, W, x, 1.5, tag=f"crafted NaN / inf {W}x{H}")
    keep = np.ones(n, bool)
    keep[[5, n - 2]] = False
    assert vals[7] == n - 2 and vals[5] == np.sort(resid[keep])[(n - 3) // 2]
    assert np.isnan(ra.reshape(-1)[[5, n - 2]]).all() and np.array_equal(ra.reshape(-1)[keep], resid[keep])
    assert not gd.reshape(-1)[[5, n - 2]].any() and not ga.reshape(-1)[[5, n - 2]].any()
    assert np.isfinite(vals).all()
    assert gi.reshape(n, 3)[[5, n - 2]].any()  # outside S_d: coupling does not reach them, their colour term stays


# ---------------------------------------------------------------------------------- 3. gate off equals the old kernel
@pytest.mark.parametrize("H,W,seed", LOSS_CASES[:3])
def test_gate_off_equals_the_ungated_kernel(gpu, H, W, seed):
    """k_d = k_c = 0: the three gradient maps and values[0:4] are gs_loss_track's with depth_gate = 0, bit for bit -- with a
    range map and without; the medians are still reported."""
    x = _inputs(H, W, seed)
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    for with_range in (True, False):
        gl = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, 0.0, 0.0, 0.0, 0.0, True, gpu, keep_residuals=True)
        gi, gd, ga, vals, ra, rc = (o.cpu().numpy() for o in _run_gated(gl, t, scale, with_range))
        pgi, pgd, pga, pvals = _run_plain(H, W, t, scale, gpu, with_range)
        for a, b in ((gi, pgi), (gd, pgd), (ga, pga), (vals[:4], pvals)):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.abs(gi).max() > 0 and (np.abs(gd).max() > 0) == with_range
        sa = np.sort(ra[~np.isnan(ra)])
        assert vals[7] == len(sa) and (len(sa) > 0) == with_range
        assert vals[5] == (sa[(len(sa) - 1) // 2] if with_range else 0.0)


def test_workspace_residual_maps_give_the_same_result(gpu):
    """keep_residuals=False (resid_depth = resid_color = NULL: the maps live in the workspace) changes nothing."""
    H, W, seed = LOSS_CASES[2]
    x = _inputs(H, W, seed)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    a = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, 1.5, 1.5, 0.0, 0.0, True, gpu, keep_residuals=True)
    b = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, 1.5, 1.5, 0.0, 0.0, True, gpu)
    assert b.resid_depth is None and b.resid_color is None
    for gl in (a, b):
        gl(*t, 0.37 / (H * W))
    for u, v in ((a.grad_image, b.grad_image), (a.grad_depth, b.grad_depth), (a.grad_alpha, b.grad_alpha), (a.values, b.values)):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------ 4. the Tracker
OCC_ROWS, OCC_COLS = slice(20, 100), slice(60, 132)  # rows 20 - 99 x columns 60 - 131: 30 % of the 160 x 120 frame


def _frame(gpu, occluded):
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    if occluded:
        img, rng = img.clone(), rng.clone()
        img[OCC_ROWS, OCC_COLS] = torch.tensor([0.9, 0.1, 0.1], device=img.device)
        rng[OCC_ROWS, OCC_COLS] *= 0.5
    return params, cam, R_true, t_true, img.contiguous(), rng.contiguous()


@pytest.mark.parametrize("leg", ["a_clean_gated", "b_occluded_gated", "c_occluded_default"])
def test_tracker_with_an_occluder(gpu, leg):
    """The case of test_tracker_recovers_a_single_frame (0.5 degrees and 0.02 off, with depth); the occluder replaces the
    target colour by (0.9, 0.1, 0.1) and halves the range over 30 % of the frame.  Gated: depth_gate_k = 10, coupled.
    (a) clean frame, gated: both errors down to a tenth -- the gate costs a clean frame nothing it needs.
    (b) occluded frame, gated: the same criterion, and at most 75 % of n_d counted.
    (c) occluded frame, default options: the control; asserts nothing about the pose, its errors are printed."""
    occluded, gated = leg != "a_clean_gated", leg != "c_occluded_default"
    params, cam, R_true, t_true, img, rng = _frame(gpu, occluded)
    before = [p.clone() for p in params]
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    opt = TrackOptions(depth_gate_k=10.0, gate_couple=True) if gated else TrackOptions()
    tr = Tracker(params, cam, opt, gpu)
    res = tr.track(img, rng, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    print(f"tracker occluder leg {leg}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, loss {res.losses[0]:.5f} -> "
          f"{res.loss:.6f}, inliers {res.inliers}, medians {res.medians}")
    for a, b in zip(before, params):
        assert torch.equal(a, b) and a.grad is None and b.grad is None  # the map is bitwise unchanged
    assert res.iterations == 300 == len(res.losses) and res.loss == min(res.losses)
    again = tr.iteration(res.rot, res.tran, img, rng)
    assert float(again[12]) == res.loss  # the loss that came back belongs to the pose that came back
    if not gated:
        assert res.inliers is None and res.medians is None and again.numel() == 16
        return
    assert again.numel() == 20
    assert res.inliers == (int(again[15]), int(again[19]), int(again[16])) and res.medians == (float(again[17]), float(again[18]))
    assert 0 < res.inliers[0] <= res.inliers[1] <= W_ * H_ and res.medians[0] > 0
    if occluded:
        assert res.inliers[0] <= 0.75 * res.inliers[1], res.inliers
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)


# ------------------------------------------------------------------------------------------------ 5. gate-off Tracker
def test_default_tracker_is_the_ungated_path(gpu):
    """Default options: Tracker.iteration returns the 16-float buffer, and on one frame its values and pose gradient are
    bitwise those of the TrackLoss path assembled by hand on a renderer of the same configuration."""
    import copy

    from gaussian import _lib
    from gs_frame import FrameRenderer

    params, cam, R_true, t_true, img, rng = _frame(gpu, False)
    R0, t0 = perturbed_start(R_true, t_true)
    o = TrackOptions()
    tr = Tracker(params, cam, o, gpu)
    assert type(tr.loss) is TrackLoss
    h = tr.iteration(R0, t0, img, rng).clone()
    assert h.numel() == 16 and tr._dev.numel() == 16
    r = FrameRenderer(gpu, max_pairs=int(o.max_pairs), training=True, occlusion_cull=False, auto_grow=True)
    c = copy.copy(cam)
    c.rot, c.tran = np.ascontiguousarray(R0, np.float32), np.ascontiguousarray(t0, np.float32)
    im, _, depth, alpha = r.forward(*params, c, training=True, aux=True)
    tl = TrackLoss(H_, W_, o.alpha_min, o.color_weight, o.depth_weight, o.depth_gate, gpu)
    gi, gd, ga = tl(im, depth, alpha, img, rng, 1.0 / (H_ * W_))
    scratch = tuple(torch.empty_like(p) for p in params)
    gp = (torch.full((3, 3), float("nan"), device=gpu), torch.full((3,), float("nan"), device=gpu))
    r.backward(gi, out=scratch, part=_lib.GS_BWD_RASTER, grad_depth=gd, grad_alpha=ga)
    r.backward(None, out=scratch, part=_lib.GS_BWD_GEOMETRY, grad_pose=gp)
    want = torch.cat([gp[0].reshape(9), gp[1], tl.values]).cpu()
    assert torch.equal(h.view(torch.int32), want.view(torch.int32))
    assert torch.isfinite(h).all() and h[0:9].abs().max() > 0 and h[12] > 0
