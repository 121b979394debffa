"""GPU tier of camera tracking against a frozen map: the loss kernel (gs_loss_track) against the fp64 evaluation and the fp32
restatement of tests/track_ref.py, its depth part bit for bit against gs_loss_depth, gs_track.Tracker on one frame (the case
of tests/test_gpu_pose.py::test_pose_recovery, without autograd) and on a sequence, and the tracker's RASTER + GEOMETRY
backward bit for bit against the one-call backward.  include/gs_abi.h states the contracts."""
import math

import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from gs_track import TrackOptions, Tracker
from gs_train import DepthLoss, TrackLoss
from track_ref import (ALPHA_MIN, GATE, LOSS_CASES, colour_grad_f32, loss_inputs, perturbed_start, pose_errors, so3_exp_series,
                       track_loss_f64)

pytestmark = pytest.mark.gpu

_INPUTS = {}


def _inputs(H, W, seed):
    """(numpy inputs, the fp64 reference at weights (0.8, 1.3) with the gate): computed once per size, never modified."""
    if (H, W) not in _INPUTS:
        x = loss_inputs(H, W, seed)
        _INPUTS[(H, W)] = (x, track_loss_f64(*x, ALPHA_MIN, 0.8, 1.3, GATE, 0.37 / (H * W)))
    return _INPUTS[(H, W)]


def _run(tl, t, scale, with_range=True):
    """One call into NaN-filled destinations -> clones of the three gradients and the four values."""
    for g in (tl.grad_image, tl.grad_depth, tl.grad_alpha):
        g.fill_(float("nan"))
    tl.values.fill_(float("nan"))
    gi, gd, ga = tl(t[0], t[1], t[2], t[3], t[4] if with_range else None, scale)
    return gi.clone(), gd.clone(), ga.clone(), tl.values.clone()


# ------------------------------------------------------------------------------------------------- 1. the loss kernel
@pytest.mark.parametrize("H,W,seed", LOSS_CASES)
def test_track_loss_matches_fp64(gpu, H, W, seed):
    """gs_loss_track against track_ref.  grad_image exactly the float32 restatement; grad_depth / grad_alpha within 1e-6 |ref|
    (the bound of test_depth_loss_matches_fp64: at most ~10 fp32 roundings of 2^-24 each); pixels whose fp64 sign of r or gate
    decision is not decidable in fp32 are left out, at most 0.1 % of the image; exact zeros where a pixel does not count; the
    depth count exact apart from the left-out pixels; the three values within 1e-5 relative; two runs bitwise equal."""
    (I, D, A, T, z), ref = _inputs(H, W, seed)
    cw, dw, scale = 0.8, 1.3, 0.37 / (H * W)
    t = [torch.from_numpy(x).to(gpu) for x in (I, D, A, T, z)]
    tl = TrackLoss(H, W, ALPHA_MIN, cw, dw, GATE, gpu)
    gi, gd, ga, vals = _run(tl, t, scale)
    gi2, gd2, ga2, vals2 = _run(tl, t, scale)
    for a, b in ((gi, gi2), (gd, gd2), (ga, ga2), (vals, vals2)):
        assert torch.equal(a, b) and not torch.isnan(a).any()  # bitwise repeatable, everything written
    # colour: exact
    assert np.array_equal(gi.cpu().numpy(), colour_grad_f32(I, T, A, ALPHA_MIN, cw, scale))
    # depth
    und, dmask = ref["undecidable"], ref["dmask"]
    share = float(und.sum()) / (H * W)
    got_gd, got_ga = gd.cpu().numpy().astype(np.float64), ga.cpu().numpy().astype(np.float64)
    check = dmask & ~und
    e_gd = float((np.abs(got_gd - ref["grad_depth"]) / np.maximum(np.abs(ref["grad_depth"]), 1e-300))[check].max())
    e_ga = float((np.abs(got_ga - ref["grad_alpha"]) / np.maximum(np.abs(ref["grad_alpha"]), 1e-300))[check].max())
    v = vals.cpu().numpy().astype(np.float64)
    print(f"track loss {W}x{H}: rel err grad_depth {e_gd:.2e} grad_alpha {e_ga:.2e}, undecidable {int(und.sum())} "
          f"(share {share:.2e}), values {v.tolist()} vs {[ref['loss'], ref['colour'], ref['depth'], ref['count']]}")
    assert share <= 1e-3
    assert e_gd <= 1e-6 and e_ga <= 1e-6
    out = ~dmask & ~und
    assert float(np.abs(got_gd[out]).max()) == 0.0 and float(np.abs(got_ga[out]).max()) == 0.0
    assert float(np.abs(gi.cpu().numpy()[~ref["cmask"]]).max()) == 0.0
    assert abs(int(v[3]) - ref["count"]) <= int(und.sum())
    for k, name in ((0, "loss"), (1, "colour"), (2, "depth")):
        # (a left-out pixel moves the depth sum by at most the gate: far inside 1e-5 of a sum over a tenth of a million)
        slack = GATE * dw * scale * int(und.sum()) if k != 1 else 0.0
        assert abs(v[k] - ref[name]) <= 1e-5 * abs(ref[name]) + slack, (name, v[k], ref[name])
    assert ref["count"] > 0.1 * H * W and ref["colour"] > 0 and ref["depth"] > 0


@pytest.mark.parametrize("H,W,seed", LOSS_CASES[:3])
def test_track_loss_rgb_only_and_isolated_terms(gpu, H, W, seed):
    """target_range = NULL: zero depth gradients and a zero depth term, the colour part unchanged.  Weights (1, 0) and (0, 1)
    each isolate their term: the other's gradients are zeros, its value is zero, and the term that remains is the fp64
    reference's at that weight."""
    (I, D, A, T, z), _ = _inputs(H, W, seed)
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(x).to(gpu) for x in (I, D, A, T, z)]
    gi, gd, ga, vals = _run(TrackLoss(H, W, ALPHA_MIN, 0.8, 1.3, GATE, gpu), t, scale, with_range=False)
    v = vals.cpu().numpy().astype(np.float64)
    ref = track_loss_f64(I, D, A, T, None, ALPHA_MIN, 0.8, 1.3, GATE, scale)
    assert not gd.any() and not ga.any() and v[2] == 0.0 and v[3] == 0.0 and v[0] == v[1]
    assert np.array_equal(gi.cpu().numpy(), colour_grad_f32(I, T, A, ALPHA_MIN, 0.8, scale))
    assert abs(v[1] - ref["colour"]) <= 1e-5 * ref["colour"]
    # colour alone
    gi, gd, ga, vals = _run(TrackLoss(H, W, ALPHA_MIN, 1.0, 0.0, GATE, gpu), t, scale)
    v = vals.cpu().numpy().astype(np.float64)
    ref = track_loss_f64(I, D, A, T, z, ALPHA_MIN, 1.0, 0.0, GATE, scale)
    assert not gd.any() and not ga.any() and v[2] == 0.0 and v[0] == v[1]
    assert np.array_equal(gi.cpu().numpy(), colour_grad_f32(I, T, A, ALPHA_MIN, 1.0, scale))
    assert abs(v[1] - ref["colour"]) <= 1e-5 * ref["colour"] and abs(int(v[3]) - ref["count"]) <= int(ref["undecidable"].sum())
    # depth alone
    gi, gd, ga, vals = _run(TrackLoss(H, W, ALPHA_MIN, 0.0, 1.0, GATE, gpu), t, scale)
    v = vals.cpu().numpy().astype(np.float64)
    ref = track_loss_f64(I, D, A, T, z, ALPHA_MIN, 0.0, 1.0, GATE, scale)
    assert not gi.any() and v[1] == 0.0 and v[0] == v[2]
    assert abs(v[2] - ref["depth"]) <= 1e-5 * ref["depth"] + GATE * scale * int(ref["undecidable"].sum())
    check = ref["dmask"] & ~ref["undecidable"]
    got = gd.cpu().numpy().astype(np.float64)
    assert float((np.abs(got - ref["grad_depth"]) / np.maximum(np.abs(ref["grad_depth"]), 1e-300))[check].max()) <= 1e-6


# -------------------------------------------------------------------------------------- 2. consistency with gs_loss_depth
@pytest.mark.parametrize("H,W,seed", LOSS_CASES[:3])
def test_depth_part_equals_the_depth_loss_kernel(gpu, H, W, seed):
    """color_weight 0, depth_weight 1, no gate, every pixel measured: the same operations in the same order as gs_loss_depth
    mode 1 (fl(scale x 1) is scale), so the two gradient maps are equal bit for bit -- and so is the depth term."""
    I, D, A, T, z = loss_inputs(H, W, seed, all_measured=True)
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(x).to(gpu) for x in (I, D, A, T, z)]
    _, gd, ga, vals = _run(TrackLoss(H, W, ALPHA_MIN, 0.0, 1.0, 0.0, gpu), t, scale)
    dl = DepthLoss(H, W, "expected", ALPHA_MIN, gpu)
    rd, ra = dl(t[1], t[2], t[4], scale)
    assert torch.equal(gd, rd) and torch.equal(ga, ra)
    assert gd.abs().max() > 0
    assert float(vals[3]) == float(dl.values[1]) and float(vals[2]) == float(dl.values[0])


# ------------------------------------------------------------------------------------------------- 3. - 5. the Tracker
W_, H_ = 160, 120
_SCENE = {}


def _scene(gpu):
    """The case of test_pose_recovery: (scene tensors, camera, a renderer for the targets), built once."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        _SCENE["x"] = (to_torch(scene, gpu), cam, FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True,
                                                                occlusion_cull=False))
    return _SCENE["x"]


def _target(gpu, rot, tran):
    """(image, range map) of the scene seen from (rot, tran): range = D / A where the map covers the pixel, else none."""
    import copy

    params, cam, r = _scene(gpu)
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    img, _, d, a = r.forward(*params, c, training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
    return img.contiguous(), rng.contiguous()


@pytest.mark.parametrize("with_depth", [False, True])
def test_tracker_recovers_a_single_frame(gpu, with_depth):
    """test_pose_recovery's case and criterion -- 0.5 degrees and 0.02 off, both errors down to a tenth -- met by the Tracker:
    no autograd, the map bitwise unchanged, the returned pose the lowest-loss one and on SO(3)."""
    params, cam, _ = _scene(gpu)
    before = [p.clone() for p in params]
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(), gpu)
    res = tr.track(img, rng if with_depth else None, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    print(f"tracker single frame depth={with_depth}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, "
          f"loss {res.losses[0]:.5f} -> {res.loss:.6f}")
    assert abs(e_r0 - math.radians(0.5)) < 1e-4 and abs(e_t0 - 0.02) < 1e-9
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    for a, b in zip(before, params):
        assert torch.equal(a, b) and a.grad is None and b.grad is None
    assert res.iterations == 300 == len(res.losses) and res.loss == min(res.losses)
    assert np.abs(res.rot @ res.rot.T - np.eye(3)).max() <= 1e-6
    # the loss that came back belongs to the pose that came back: the frame is a pure function of its inputs
    again = float(tr.iteration(res.rot, res.tran, img, rng if with_depth else None)[12])
    assert again == res.loss


def test_tracker_follows_a_sequence(gpu):
    """Six views along an arc, 0.5 degrees and 0.02 per frame (a constant twist in the camera frame), targets rendered from
    the true poses, track() per frame without `init`: the first frame starts at the constructor camera's pose, the second
    from the first's, the others from the constant-velocity prediction.  From the third frame on both errors are at most a
    tenth of the motion since the frame before."""
    params, cam, _ = _scene(gpu)
    rng_ = np.random.default_rng(211)
    axis = rng_.normal(size=3)
    axis /= np.linalg.norm(axis)
    dR = so3_exp_series(axis * math.radians(0.5))
    u = rng_.normal(size=3)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * 0.02 - (dR @ t - t)  # (the first step moves tran by 0.02 exactly, the others within 2 %)
    poses = [(R, t)]
    for _ in range(5):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    motion = [None] + [pose_errors(*poses[k], *poses[k - 1]) for k in range(1, 6)]
    tr = Tracker(params, cam, TrackOptions(), gpu)
    errs = []
    for R, t in poses:
        img, rng = _target(gpu, R, t)
        res = tr.track(img, rng)
        errs.append(pose_errors(res.rot, res.tran, R, t))
    print("tracker sequence: motion per frame " + ", ".join(f"({a:.3e}, {b:.3e})" for a, b in motion[1:])
          + "; errors after tracking " + ", ".join(f"({a:.2e}, {b:.2e})" for a, b in errs))
    for k in range(1, 6):
        assert abs(motion[k][0] - math.radians(0.5)) < 1e-4 and abs(motion[k][1] - 0.02) < 0.02 * 0.02
    for k in range(2, 6):
        assert errs[k][0] <= 0.1 * motion[k][0] and errs[k][1] <= 0.1 * motion[k][1], (k, errs)
    tr.reset()
    assert tr._start_pose(None)[0].tolist() == cam.rot.astype(np.float64).tolist()


def test_tracker_iteration_equals_the_one_call_backward(gpu):
    """The pose gradient of one Tracker iteration (RASTER part, then GEOMETRY part with grad_pose; the COLOR part never run)
    is, bit for bit, that of the one-call backward fed the same three gradient maps on the same frame."""
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(), gpu)
    h = tr.iteration(R0, t0, img, rng).clone()
    gp = (torch.full((3, 3), float("nan"), device=gpu), torch.full((3,), float("nan"), device=gpu))
    tr.renderer.backward(tr.loss.grad_image, grad_depth=tr.loss.grad_depth, grad_alpha=tr.loss.grad_alpha, grad_pose=gp)
    assert torch.equal(h[0:9], gp[0].reshape(9).cpu()) and torch.equal(h[9:12], gp[1].cpu())
    assert torch.isfinite(h).all() and h[0:9].abs().max() > 0 and h[9:12].abs().max() > 0
    # (loss = colour + depth in double, each of the three rounded to fp32 once)
    assert h[12] > 0 and h[15] > 0 and abs(float(h[12]) - (float(h[13]) + float(h[14]))) <= 3 * 2.0 ** -24 * float(h[12])
