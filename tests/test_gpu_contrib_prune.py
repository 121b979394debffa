"""GPU tier of visibility pruning: Trainer.contributions / Trainer.prune(contributions=...) on a three-view fit of an opaque wall
with Gaussians planted behind it and outside every frustum, and gs_slam.Slam with ``prune_unseen_every`` on the eight-frame arc
of tests/test_gpu_slam.py (its helpers are restated here).

The wall: 12 x 9 Gaussians of sigma 6 pixels, 9 pixels apart, opacity logit 10, well inside all three 160 x 120 views.  Behind
the centre of each of them nothing gets through: alpha there is 0.99995, and 0.3 pixels off the centre still 0.9987, so a
small (sigma 0.3 pixels) Gaussian of opacity 0.011 (logit -4.5: above 1/255, it would be seen in the open) planted right behind
a centre has w <= 0.011 x 3e-4 everywhere -- far below 1/255, and below the image tolerance 5e-5 that the re-rendered views
are held to.  The fit runs at a tenth of the default rates: Adam normalises the planted rows' tiny gradients, so at the default
rates six steps double their extent and carry them out from behind the centres, where they do become visible.  No wall
Gaussian is buried: at its own centre each has at least 0.68^4 0.9^4 = 0.14 of the transmittance left whatever the depth order
of its neighbours."""
import copy
import math

import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_scene import Scene, make_camera
from gs_testutil import aux_case, to_torch
from gs_train import TrainOptions, Trainer
from track_ref import pose_errors, so3_exp_series

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
F_ = 0.75 * W_
NAMES = ("pos", "quat", "scale", "opa", "rgb")
N_BEHIND, N_OUTSIDE = 200, 200


def _wall_scene():
    """-> (scene, planted mask).  Pixel coordinates are those of the unyawed view at the origin."""
    g = np.random.default_rng(41)
    rows = []

    def add(px, py, z, sigma_px, logit):
        rows.append(((px - W_ / 2) / F_ * z, (py - H_ / 2) / F_ * z, z, max(sigma_px * abs(z) / F_ - 1e-4, 1e-6), logit))

    centres = [(80 + 9 * (i - 5.5), 60 + 9 * (j - 4)) for j in range(9) for i in range(12)]
    for px, py in centres:
        add(px, py, 4.0 + g.uniform(-0.02, 0.02), 6.0, 10.0)
    n_wall = len(rows)
    for k in range(N_BEHIND):  # right behind wall centres (two per centre at most, at different depths)
        px, py = centres[k % len(centres)]
        add(px, py, 5.0 + 0.5 * (k // len(centres)), 0.3, -4.5)
    for k in range(N_OUTSIDE):  # outside every frustum: far to the side, or behind the cameras
        if k % 2:
            add(g.uniform(0, W_), g.uniform(0, H_), -g.uniform(0.5, 5.0), 4.0, 2.0)
        else:
            rows.append((g.choice([-1.0, 1.0]) * g.uniform(40.0, 60.0), g.uniform(-2, 2), 4.0, 0.1, 2.0))
    a = np.array(rows, np.float64)
    n = a.shape[0]
    quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    scene = Scene(a[:, 0:3].astype(np.float32), quat.astype(np.float32), np.repeat(a[:, 3:4], 3, 1).astype(np.float32),
                  a[:, 4].astype(np.float32), g.uniform(-2.0, 2.0, (n, 3)).astype(np.float32))
    planted = np.arange(n) >= n_wall
    return scene, planted


def _fit(gpu, steps=5):
    scene, planted = _wall_scene()
    cams = []
    for yaw, tx in ((0.0, 0.0), (-3.0, -0.02), (3.0, 0.02)):  # (0.02: a parallax of 0.12 pixels behind the wall)
        c = make_camera(W_, H_, yaw_deg=yaw)
        c.tran = np.array([tx, 0.0, 0.0], np.float32)
        cams.append(c)
    start = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 18, auto_grow=True)
    targets = [(r.forward(*start, cam, training=False)[0] + 0.05).clamp(0, 1).contiguous().clone() for cam in cams]
    tr = Trainer([t.clone() for t in start], cams, targets, TrainOptions(n_iters=51, n_iters_warmup=3, lr=0.0003), max_pairs=1 << 18)
    for i in range(steps):
        tr.train_step(i, i % 3)
    return tr, torch.from_numpy(planted).to(gpu)


def _state(tr):
    o = tr.optimizer
    return [tr.flat.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.accum_grad.clone()]


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(_state(a), _state(b))) \
        and a.optimizer.step_count == b.optimizer.step_count


def _render_all(gpu, tr):
    r = FrameRenderer(gpu, max_pairs=1 << 18, auto_grow=True)
    return [r.forward(*tr.flat.params, cam, training=False)[0].clone() for cam in tr.cameras]


def test_trainer_contributions_and_the_prune_of_what_no_view_sees(gpu):
    a, planted = _fit(gpu)
    b, _ = _fit(gpu)
    c, _ = _fit(gpu)
    assert _same(a, b) and _same(a, c) and a.optimizer.exp_avg.abs().max() > 0
    n = a.n_gaussians
    # a train_step after contributions() alone is the step without it, bit for bit
    seen = a.contributions()
    la, lc = a.train_step(5, 2).clone(), c.train_step(5, 2).clone()
    assert _same(a, c) and torch.equal(la, lc)
    b.train_step(5, 2)
    seen = a.contributions()
    assert tuple(seen.rows.shape) == (n, 4) and seen.w_min == 1.0 / 255.0
    views = seen.views
    assert int(views.max()) == 3 and not bool(views[planted].any())  # every planted row: seen by no view
    per_view = [a.contributions([k]) for k in range(3)]
    wall_seen = torch.stack([p.weight_max >= 0.05 for p in per_view]).any(0)
    assert int(wall_seen.sum()) == n - int(planted.sum()) and bool((views[wall_seen] > 0).all())  # the whole wall is seen
    assert torch.equal(views, per_view[0].views + per_view[1].views + per_view[2].views)
    assert torch.equal(seen.weight_max, torch.stack([p.weight_max for p in per_view]).max(0).values)
    unseen = views == 0
    assert torch.equal(unseen, planted)
    before = _render_all(gpu, a)
    # (a) the kernel path
    flat_a, opt_a = a.flat, a.optimizer
    removed = a.prune(6, contributions=seen, views_min=1)
    assert removed == int(unseen.sum()) == N_BEHIND + N_OUTSIDE and a.n_gaussians == n - removed
    assert a.flat is not flat_a and a.optimizer is not opt_a
    # (b) the torch assembly (tests/test_gpu_prune.py): a plain rebind, moments and statistic by boolean indexing
    mask = ~unseen
    old = [p.clone() for p in b.flat.params]
    moments = {name: [m.clone() for m in b.optimizer.moment_rows(name)] for name in NAMES}
    stat, steps = b.optimizer.accum_grad.clone(), b.optimizer.step_count
    b._bind([p[mask] for p in old], 6)
    for name in NAMES:
        for dst, src in zip(b.optimizer.moment_rows(name), moments[name]):
            dst.copy_(src[mask])
    b.optimizer.accum_grad.copy_(stat[mask])
    b.optimizer.step_count = steps
    assert steps == 6 and _same(a, b)
    # every training view, re-rendered: the image tolerance
    after = _render_all(gpu, a)
    errs = [float((x - y).abs().max()) for x, y in zip(before, after)]
    print(f"prune of {removed} unseen rows out of {n}: image max |diff| per view " + ", ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= 5e-5
    la, lb = a.train_step(6, 0).clone(), b.train_step(6, 0).clone()
    assert _same(a, b) and torch.equal(la, lb) and a.optimizer.step_count == 7
    # joined to the opacity rule; a row count that does not match is refused; nothing unseen is left
    with pytest.raises(RuntimeError):
        a.prune(7, contributions=seen, views_min=1)
    again = a.contributions()
    assert a.prune(7, contributions=again, views_min=1) == 0
    assert a.prune(7, opa_min=0.5, contributions=again, views_min=1, carry_state=False) == int((a.flat.params[3] <= 0).sum())


# ------------------------------------------------------------------------------------------------------------------ Slam
N_FRAMES = 8


def _posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def _arc(gpu, n=N_FRAMES):
    """The arc of tests/test_gpu_slam.py: the 20,000-Gaussian truth scene, 0.5 degrees and 0.02 per frame."""
    scene, cam = aux_case(20_000, W_, H_, seed=103)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False)
    rng_ = np.random.default_rng(211)
    axis = rng_.normal(size=3)
    axis /= np.linalg.norm(axis)
    dR = so3_exp_series(axis * math.radians(0.5))
    u = rng_.normal(size=3)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * 0.02 - (dR @ t - t)
    poses = [(R, t)]
    for _ in range(n - 1):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    targets = []
    for R, t in poses:
        img, _, d, a = r.forward(*params, _posed(cam, R, t), training=False, aux=True)
        rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
        targets.append((img.contiguous().clone(), rng.contiguous().clone()))
    return cam, poses, targets


def test_the_loop_prunes_what_no_keyframe_sees(gpu):
    """prune_unseen_every = 1 on the eight-frame arc (keyframes at frames 0, 3 and 6): ``pruned_unseen`` is the drop in the
    Gaussian count, the losses stay finite, the tracker stays bound to the trainer's tensors, and from frame 2 on both pose
    errors of every frame are at most the motion since the previous frame (the criterion of tests/test_gpu_slam.py)."""
    from gs_slam import Slam, SlamOptions

    cam, poses, targets = _arc(gpu)
    slam = Slam(_posed(cam, *poses[0]), SlamOptions(overlap_min=0.0, keyframe_every=3, prune_unseen_every=1), gpu)
    rows = []
    for f, ((R, t), (img, rng)) in enumerate(zip(poses, targets)):
        frame = slam.begin(img, rng)
        n_seeded = slam.trainer.n_gaussians
        assert slam.map(frame) is frame
        tr = slam.trainer
        assert frame.pruned_unseen == n_seeded - tr.n_gaussians and frame.pruned == 0
        assert ("prune_unseen" in frame.seconds) == frame.keyframe
        assert all(a.data_ptr() == b.data_ptr() and a.shape == b.shape for a, b in zip(slam.tracker.params, tr.flat.params))
        if frame.keyframe:  # nothing unseen is left behind the prune
            assert not bool((tr.contributions().views == 0).any())
        err = pose_errors(frame.rot, frame.tran, R, t)
        motion = pose_errors(*poses[f], *poses[f - 1]) if f else None
        rows.append((frame, err, motion))
        print(f"  frame {f}: keyframe {frame.keyframe} added {frame.added} pruned_unseen {frame.pruned_unseen} Gaussians "
              f"{tr.n_gaussians} pose error ({err[0]:.3e}, {err[1]:.3e}) motion {motion}")
    assert [fr.keyframe for fr, _, _ in rows] == [True, False, False, True, False, False, True, False]
    assert sum(fr.pruned_unseen for fr, _, _ in rows) > 0
    assert all(math.isfinite(v) for fr, _, _ in rows for v in fr.map_losses)
    for f in range(2, N_FRAMES):
        _, err, mo = rows[f]
        assert err[0] <= mo[0] and err[1] <= mo[1], (f, err, mo)


def test_the_option_is_off_by_default(gpu, monkeypatch):
    """With prune_unseen_every = 0 the loop never asks for contributions and never prunes (both are patched to raise), on a
    four-frame prefix of the arc with a few mapping steps; and two such runs end in the same poses and the same map, bit for
    bit.  What is compared is the new code with itself: that the run equals the parent commit's follows from the calls not
    being issued -- the option adds one `if` to ``Slam.map`` -- and is not measured against the parent's code here."""
    from gs_slam import Slam, SlamOptions

    def refuse(*a, **k):
        raise AssertionError("Trainer.contributions / Trainer.prune called with the option off")

    monkeypatch.setattr(Trainer, "contributions", refuse)
    monkeypatch.setattr(Trainer, "prune", refuse)
    cam, poses, targets = _arc(gpu, 4)
    runs = []
    for _ in range(2):
        slam = Slam(_posed(cam, *poses[0]), SlamOptions(overlap_min=0.0, keyframe_every=3, map_iterations_first=6,
                                                       map_iterations=4), gpu)
        frames = [slam.step(*t) for t in targets]
        assert [fr.pruned_unseen for fr in frames] == [0, 0, 0, 0] and all("prune_unseen" not in fr.seconds for fr in frames)
        runs.append((frames, slam.trainer.flat.flat_param.clone(), slam.trainer.optimizer.step_count, slam.i_iter))
    assert runs[0][2:] == runs[1][2:] == (4, 10) and torch.equal(runs[0][1], runs[1][1])
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x.rot, y.rot) and np.array_equal(x.tran, y.tran) and x.map_losses == y.map_losses
