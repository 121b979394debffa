"""GPU tier of the exposure fit in tracking and mapping (TrackOptions.fit_exposure, SlamOptions through .track and
.refine_exposure): the six numbers recovered at the true pose, pose and exposure recovered together on the frame of
tests/test_gpu_track.py, the unaltered frame left alone, a coarse-to-fine schedule, and every option-off path bit for bit the
call sequence it was.  The altered exposure is exposure_ref.GAIN_STAR / BIAS_STAR, applied with the restatement.

The criterion for the six numbers is the project's tracking criterion: each error at most a tenth of its scale
(exposure_ref.tenth_scales: the number's own starting error from the identity; the one bias that starts with no error takes
the smallest scale of its group)."""
import copy
import math

import numpy as np
import pytest
import torch

import exposure_ref as X
from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from gs_track import TrackOptions, Tracker
from track_ref import perturbed_start, pose_errors, so3_exp_series

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
_SCENE = {}
STAR = np.asarray(X.GAIN_STAR + X.BIAS_STAR, np.float64)
IDENT = np.asarray([1, 1, 1, 0, 0, 0], np.float64)


def _scene(gpu):
    """The case of tests/test_gpu_track.py: (scene tensors, camera, a renderer for the targets), built once."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        _SCENE["x"] = (to_torch(scene, gpu), cam, FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True,
                                                                occlusion_cull=False))
    return _SCENE["x"]


def _posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def _target(gpu, rot, tran, altered):
    """(image, range map) of the scene seen from (rot, tran), the image through the altered exposure when asked."""
    params, cam, r = _scene(gpu)
    img, _, d, a = r.forward(*params, _posed(cam, rot, tran), training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous().clone()
    img = img.contiguous().clone()
    if altered:
        img = torch.from_numpy(X.apply(img.cpu().numpy(), X.numbers(X.GAIN_STAR, X.BIAS_STAR))).to(gpu)
    return img, rng


def _numbers(res):
    return np.concatenate(res.exposure)


def _colour_term(tr, res, img, rng):
    """The colour term of the returned pose under the returned exposure: one more iteration, nothing steps."""
    if tr._exposures is not None:
        next(iter(tr._exposures.values())).set(*res.exposure)
    return float(tr.iteration(res.rot, res.tran, img, rng)[13])


def test_exposure_only_fit_at_the_true_pose(gpu):
    """The target is the tracker's own render at the true pose through (gain*, bias*), built with the restatement: the colour
    loss at (gain*, bias*) is exactly zero.  Pose rates 0, RGB only, the default exposure rates: from the identity every one
    of the six errors ends at most a tenth of its scale, and the pose has not moved.  These rates are TrackOptions'
    defaults."""
    params, cam, _ = _scene(gpu)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    o = TrackOptions(lr_rot=0.0, lr_tran=0.0, fit_exposure=True)
    assert (o.lr_gain, o.lr_bias) == (TrackOptions().lr_gain, TrackOptions().lr_bias)
    tr = Tracker(params, cam, o, gpu)
    img, _, _, _ = tr.renderer.forward(*params, _posed(cam, R, t), training=True, aux=True)
    render = img.contiguous().clone()
    target = torch.from_numpy(X.apply(render.cpu().numpy(), X.numbers(X.GAIN_STAR, X.BIAS_STAR))).to(gpu)
    res = tr.track(target, None, init=(R, t))
    got = _numbers(res)
    err, start, scales = np.abs(got - STAR), np.abs(IDENT - STAR), X.tenth_scales()
    print(f"exposure-only fit: loss {res.losses[0]:.6f} -> {res.loss:.3e}; numbers {got.tolist()}; errors {err.tolist()} "
          f"from {start.tolist()}; err / scale {(err / scales).tolist()}")
    assert (err <= 0.1 * scales).all(), (err, scales)
    assert res.loss < 0.05 * res.losses[0] and res.iterations == 300
    assert np.array_equal(res.rot, R) and np.array_equal(res.tran, t)
    # at (gain*, bias*) itself the colour loss is exactly zero, and the fit starts where it is told to
    ex = tr._exposures[0]
    ex.set(X.GAIN_STAR, X.BIAS_STAR)
    assert float(tr.iteration(R, t, target, None)[12]) == 0.0
    res2 = tr.track(target, None, init=(R, t), init_exposure=(X.GAIN_STAR, X.BIAS_STAR))
    assert res2.loss == 0.0 and res2.losses[0] == 0.0
    assert np.array_equal(_numbers(res2), X.numbers(X.GAIN_STAR, X.BIAS_STAR).astype(np.float64))


@pytest.mark.parametrize("with_depth", [False, True])
def test_joint_fit_of_pose_and_exposure(gpu, with_depth):
    """The frame of test_tracker_recovers_a_single_frame -- 0.5 degrees and 0.02 off -- with the altered target: with the
    option both pose errors and all six exposure errors come down to a tenth; the same call without the option is the
    control, whose final colour loss is higher (its pose errors are printed, not asserted)."""
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true, altered=True)
    rng = rng if with_depth else None
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(fit_exposure=True), gpu)
    res = tr.track(img, rng, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    err, scales = np.abs(_numbers(res) - STAR), X.tenth_scales()
    colour = _colour_term(tr, res, img, rng)
    ctl = Tracker(params, cam, TrackOptions(), gpu)
    cres = ctl.track(img, rng, init=(R0, t0))
    c_r, c_t = pose_errors(cres.rot, cres.tran, R_true, t_true)
    c_colour = _colour_term(ctl, cres, img, rng)
    print(f"joint fit depth={with_depth}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, loss {res.losses[0]:.5f} -> "
          f"{res.loss:.6f} (colour {colour:.6f}), exposure {_numbers(res).tolist()} err / scale {(err / scales).tolist()}; "
          f"control without the option: rot -> {c_r:.3e}, tran -> {c_t:.3e}, loss {cres.losses[0]:.5f} -> {cres.loss:.6f} "
          f"(colour {c_colour:.6f})")
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    assert (err <= 0.1 * scales).all(), (err, scales)
    assert c_colour > colour
    assert cres.exposure is None and res.exposure is not None and res.iterations == 300


def test_unaltered_target_keeps_the_identity(gpu):
    """The option on a frame whose exposure did not change: the pose criterion still holds and the six numbers end within a
    tenth of the same scales of the identity."""
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true, altered=False)
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(fit_exposure=True), gpu)
    res = tr.track(img, rng, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    err, scales = np.abs(_numbers(res) - IDENT), X.tenth_scales()
    print(f"unaltered target: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, exposure {_numbers(res).tolist()} "
          f"err / scale {(err / scales).tolist()}")
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    assert (err <= 0.1 * scales).all(), (err, scales)
    # the next call starts from this frame's exposure; reset() forgets it
    assert np.array_equal(tr._last_exposure.astype(np.float64), _numbers(res))
    tr.reset()
    assert tr._last_exposure is None


def test_schedule_runs_and_option_off_is_the_call_sequence_it_was(gpu):
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true, altered=True)
    R0, t0 = perturbed_start(R_true, t_true)
    n = 12
    tr = Tracker(params, cam, TrackOptions(fit_exposure=True, pyramid=((1, n), (0, n))), gpu)
    assert sorted(tr._exposures) == [0, 1] and tr._exposures[0].numbers.data_ptr() == tr._exposures[1].numbers.data_ptr()
    assert tr._exposures[1].out.shape == (H_ // 2, W_ // 2, 3) and tr._host.numel() == 22
    res = tr.track(img, rng, init=(R0, t0))
    assert res.levels == [(1, 0, n), (0, n, n)] and res.iterations == 2 * n and all(math.isfinite(x) for x in res.losses)
    gain, bias = res.exposure
    assert gain.shape == (3,) and bias.shape == (3,) and (gain < 1).all()  # every gain has left the identity downwards
    # option off: a tracker built with default options and one told fit_exposure=False explicitly issue the same calls
    a = Tracker(params, cam, TrackOptions(iterations=n), gpu)
    b = Tracker(params, cam, TrackOptions(iterations=n, fit_exposure=False, lr_gain=0.5, lr_bias=0.5), gpu)
    assert a._exposures is None and b._exposures is None and a._host.numel() == 16 == b._host.numel()
    ra, rb = a.track(img, rng, init=(R0, t0)), b.track(img, rng, init=(R0, t0))
    assert ra.losses == rb.losses and ra.exposure is None and rb.exposure is None
    assert np.array_equal(ra.rot, rb.rot) and np.array_equal(ra.tran, rb.tran)
    with pytest.raises(ValueError, match="init_exposure needs"):
        a.track(img, rng, init=(R0, t0), init_exposure=((1, 1, 1), (0, 0, 0)))


# ------------------------------------------------------------------------------------------------------------------ Slam
def _arc(cam, n):
    """The arc of test_tracker_follows_a_sequence: a constant twist in the camera frame, 0.5 degrees and 0.02 per frame."""
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
    return poses


def _slam_options(**kw):
    from gs_slam import SlamOptions

    return SlamOptions(overlap_min=0.0, **kw)  # keyframes by the forced interval alone


def test_slam_carries_the_tracked_exposure_into_mapping(gpu):
    """Two frames of the arc, the second through the altered exposure, both keyframes.  With track.fit_exposure the second
    keyframe's exposure meets the tenth criterion and enters the trainer fixed; keyframe 0 has no exposure.  Keyframe 0's
    colour loss (mean |render - target| of the uncompensated evaluation render) after the second keyframe's mapping steps is
    no higher than in the same run without the option, where the darker frame is baked into the shared Gaussians."""
    from gs_slam import Slam

    _, cam, _ = _scene(gpu)
    poses = _arc(cam, 2)
    frames = [_target(gpu, *poses[0], altered=False), _target(gpu, *poses[1], altered=True)]
    out = {}
    for fit in (True, False):
        # (120 steps on the first frame: SlamOptions' own figure for a keyframe that ends below its seeded loss -- the six
        # numbers are fitted against the map, and what the map has not learnt of frame 0 they absorb)
        opt = _slam_options(keyframe_every=1, map_iterations_first=120, map_iterations=60,
                            track=TrackOptions(fit_exposure=fit))
        slam = Slam(_posed(cam, *poses[0]), opt, gpu)
        f0 = slam.step(*frames[0])
        f1 = slam.step(*frames[1])
        assert f0.keyframe and f1.keyframe and f0.exposure is None and f1.window[0] == 1 and 0 in f1.window
        shown = slam.trainer.test(0)["image"]
        out[fit] = (f1, float((shown - frames[0][0]).abs().mean()), slam)
    f1, loss0, slam = out[True]
    err, scales = np.abs(np.concatenate(f1.exposure) - STAR), X.tenth_scales()
    print(f"slam exposure: keyframe 1 exposure {np.concatenate(f1.exposure).tolist()} err / scale {(err / scales).tolist()}; "
          f"keyframe 0 colour loss after keyframe 1's mapping: {loss0:.6f} with the option, {out[False][1]:.6f} without; "
          f"pose errors {pose_errors(f1.rot, f1.tran, *poses[1])} with, {pose_errors(out[False][0].rot, out[False][0].tran, *poses[1])} "
          f"without")
    assert (err <= 0.1 * scales).all(), (err, scales)
    assert sorted(slam.trainer._exposure) == [1] and not slam.trainer._exposure[1].is_free
    got = slam.trainer.exposure(1)
    assert np.array_equal(np.concatenate(got), np.concatenate(f1.exposure))  # held fixed through the mapping steps
    assert out[False][0].exposure is None and not out[False][2].trainer._exposure
    assert loss0 <= out[False][1]


def test_slam_refine_exposure_frees_the_window_but_never_keyframe_0(gpu):
    from gs_slam import Slam

    _, cam, _ = _scene(gpu)
    poses = _arc(cam, 2)
    frames = [_target(gpu, *poses[0], altered=False), _target(gpu, *poses[1], altered=True)]
    opt = _slam_options(keyframe_every=1, map_iterations_first=8, map_iterations=20, refine_exposure=True,
                        track=TrackOptions(fit_exposure=True, iterations=100))
    slam = Slam(_posed(cam, *poses[0]), opt, gpu)
    slam.step(*frames[0])
    frame = slam.begin(*frames[1])
    tracked = np.concatenate(frame.exposure)
    slam.map(frame)
    refined = np.concatenate(frame.exposure)
    assert sorted(slam.trainer._exposure) == [1] and not slam.trainer._exposure[1].is_free  # freed, stepped, fixed again
    # view 1 takes 10 of the 20 round-robin steps; one Adam step moves a number by at most lr (1 - b1) / sqrt(1 - b2) = 3.17 lr
    assert not np.array_equal(tracked, refined) and np.abs(refined - tracked).max() <= 10 * 3.17 * opt.exposure_lr_gain
    assert np.array_equal(slam.tracker._last_exposure.astype(np.float64), refined)


def test_with_everything_off_the_loop_is_the_call_sequence_it_was(gpu):
    """The comparison of tests/test_gpu_slam_icp.py for icp = None: a two-frame run with the options off -- given explicitly --
    returns the poses and losses of the calls the loop issued before the options existed, made by hand, bit for bit."""
    import gs_seed
    from gs_slam import Slam
    from gs_train import Trainer

    _, cam, _ = _scene(gpu)
    poses = _arc(cam, 2)
    targets = [_target(gpu, *poses[0], altered=False), _target(gpu, *poses[1], altered=True)]
    opt = _slam_options(keyframe_every=1000, map_iterations_first=8, refine_exposure=False,
                        track=TrackOptions(fit_exposure=False))
    slam = Slam(_posed(cam, *poses[0]), opt, gpu)
    slam.step(*targets[0])
    frame = slam.step(*targets[1])
    assert frame.exposure is None and not frame.keyframe and not slam.trainer._exposure and slam._gate_exposure is None

    cam0 = _posed(cam, *poses[0])
    cam0 = slam._posed(np.asarray(cam0.rot, np.float64), np.asarray(cam0.tran, np.float64))
    seed = {k: v for k, v in opt.seed.items() if k != "color_dim"}
    params = gs_seed.seed_from_depth(targets[0][0], targets[0][1], cam0, color_dim=3, **seed)
    trainer = Trainer(params, [cam0], [targets[0][0]], opt.train, max_pairs=int(opt.max_pairs), depths=[targets[0][1]])
    for i in range(8):
        trainer.train_step(i, 0)
    tracker = Tracker(trainer.flat.params, cam0, TrackOptions(), gpu)
    res = tracker.track(*targets[1])
    assert np.array_equal(frame.rot.view(np.uint64), res.rot.view(np.uint64))
    assert np.array_equal(frame.tran.view(np.uint64), res.tran.view(np.uint64))
    assert frame.tracked.losses == res.losses
    for a, b in zip(slam.params, trainer.flat.params):
        assert torch.equal(a, b)
