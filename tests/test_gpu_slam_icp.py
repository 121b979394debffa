"""GPU tier of the depth alignment inside the mapping loop (gs_slam.SlamOptions.icp): the eight-frame arc of
tests/test_gpu_slam.py (its scene, arc and helpers restated here) with the ICP stage in front of the tracker, and the loop
without the option against the call sequence it always issued."""
import copy
import math

import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from track_ref import pose_errors, so3_exp_series

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
N_FRAMES = 8
_SCENE, _RUN = {}, {}


def _scene(gpu):
    """The truth map: (scene tensors, camera, a renderer for the targets), built once."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        _SCENE["x"] = (to_torch(scene, gpu), cam, FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True,
                                                                occlusion_cull=False))
    return _SCENE["x"]


def _posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def _target(gpu, rot, tran):
    """(image, range map) of the truth scene seen from (rot, tran): range = D / A where the map covers the pixel, else none."""
    params, cam, r = _scene(gpu)
    img, _, d, a = r.forward(*params, _posed(cam, rot, tran), training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
    return img.contiguous().clone(), rng.contiguous().clone()


def _poses(cam, n):
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


def _frames(gpu):
    if "frames" not in _RUN:
        _, cam, _ = _scene(gpu)
        poses = _poses(cam, N_FRAMES)
        _RUN["frames"] = (poses, [_target(gpu, R, t) for R, t in poses])
    return _RUN["frames"]


def _options(**kw):
    from gs_slam import SlamOptions

    return SlamOptions(overlap_min=0.0, **kw)  # keyframes by the forced interval alone: the schedule is known


def _run(gpu):
    """Eight frames through Slam with keyframe_every = 3 and the default IcpOptions, observed: what the tracker was started
    from is recorded per frame.  Run once."""
    if "slam" in _RUN:
        return _RUN["slam"]
    from gs_icp import IcpOptions
    from gs_slam import Slam

    _, cam, _ = _scene(gpu)
    poses, targets = _frames(gpu)
    slam = Slam(_posed(cam, *poses[0]), _options(keyframe_every=3, icp=IcpOptions()), gpu)
    rows = []
    for f, ((R, t), (img, rng)) in enumerate(zip(poses, targets)):
        seen = {}
        if slam.tracker is not None:
            real = slam.tracker.track
            seen["prediction"] = slam.tracker._start_pose(None)

            def spy(image, range_map=None, init=None, _real=real, _seen=seen):
                _seen["init"] = init
                return _real(image, range_map, init)

            slam.tracker.track = spy
        before = [p.clone() for p in slam.params] if slam.params is not None else None
        frame = slam.begin(img, rng)
        if slam.tracker is not None and "track" in slam.tracker.__dict__:
            del slam.tracker.track
        # the stage reads the map and writes nothing: a frame that is no keyframe leaves the parameters bit for bit
        untouched = before is not None and not frame.keyframe and all(torch.equal(a, b) for a, b in zip(before, slam.params))
        slam.map(frame)
        rows.append(dict(frame=frame, err=pose_errors(frame.rot, frame.tran, R, t), seen=seen, untouched=untouched))
    motion = [None] + [pose_errors(*poses[k], *poses[k - 1]) for k in range(1, N_FRAMES)]
    print("slam sequence with icp, 160 x 120, keyframe_every 3 (rotation error, translation error):")
    for f, row in enumerate(rows):
        fr = row["frame"]
        if fr.icp is None:
            print(f"  frame {f}: first frame")
            continue
        ie = pose_errors(fr.icp.rot, fr.icp.tran, *poses[f])
        pe = pose_errors(*row["seen"]["prediction"], *poses[f])
        print(f"  frame {f}: prediction ({pe[0]:.3e}, {pe[1]:.3e}) icp ({ie[0]:.3e}, {ie[1]:.3e}) accepted {fr.icp.accepted} "
              f"inliers {fr.icp.inliers} / {fr.icp.measured} rmse {fr.icp.rmse:.3e} -> slam ({row['err'][0]:.3e}, "
              f"{row['err'][1]:.3e}) motion ({motion[f][0]:.3e}, {motion[f][1]:.3e}) icp {fr.seconds['icp'] * 1e3:.2f} ms track "
              f"{fr.seconds['track'] * 1e3:.1f} ms")
    _RUN["slam"] = dict(slam=slam, rows=rows, motion=motion)
    return _RUN["slam"]


def test_every_later_frame_is_aligned_before_it_is_tracked(gpu):
    from gs_icp import IcpResult

    run = _run(gpu)
    assert run["slam"].aligner is not None
    first = run["rows"][0]["frame"]
    assert first.icp is None and "icp" not in first.seconds
    for f in range(1, N_FRAMES):
        row = run["rows"][f]
        fr, seen = row["frame"], row["seen"]
        assert isinstance(fr.icp, IcpResult) and fr.icp.iterations == 19 and fr.icp.log.shape == (19, 40)
        assert fr.seconds["icp"] > 0 and fr.tracked is not None
        assert fr.tracked.iterations == run["slam"].opt.track.iterations  # the photometric count stays the caller's
        if fr.icp.accepted:
            assert seen["init"] is not None
            assert np.array_equal(seen["init"][0], fr.icp.rot) and np.array_equal(seen["init"][1], fr.icp.tran)
        else:
            # declined: the tracker starts where it would have started -- its own prediction -- and the result carries it
            assert seen["init"] is None
            rot_p, tran_p = seen["prediction"]
            assert np.abs(fr.icp.rot - rot_p).max() < 1e-6 and np.abs(fr.icp.tran - tran_p).max() < 1e-6
        assert row["untouched"] == (f not in (3, 6)), f
    assert [f for f, row in enumerate(run["rows"]) if row["frame"].keyframe] == [0, 3, 6]


def test_tracking_still_helps_with_icp(gpu):
    """The criterion of tests/test_gpu_slam.py::test_tracking_helps, unchanged: from frame 2 on, both pose errors of every
    frame are at most the motion since the previous frame."""
    run = _run(gpu)
    for f in range(1, N_FRAMES):
        assert abs(run["motion"][f][0] - math.radians(0.5)) < 1e-4 and abs(run["motion"][f][1] - 0.02) < 0.02 * 0.02
    for f in range(2, N_FRAMES):
        err, mo = run["rows"][f]["err"], run["motion"][f]
        assert err[0] <= mo[0] and err[1] <= mo[1], (f, err, mo)


def test_without_icp_the_loop_is_the_call_sequence_it_was(gpu):
    """icp = None (the default): no aligner, no renderer for it, and a two-frame run -- the options of
    test_a_frame_that_is_no_keyframe_leaves_the_map_alone -- returns the poses of the calls the loop issued before the option
    existed, made by hand: seed, Trainer, eight mapping steps, Tracker.track, bit for bit."""
    import gs_seed
    from gs_slam import Slam
    from gs_track import Tracker
    from gs_train import Trainer

    _, cam, _ = _scene(gpu)
    poses, targets = _frames(gpu)
    opt = _options(keyframe_every=1000, map_iterations_first=8)
    assert opt.icp is None
    slam = Slam(_posed(cam, *poses[0]), opt, gpu)
    assert slam.aligner is None and slam._icp_renderer is None
    slam.step(*targets[0])
    frame = slam.step(*targets[1])
    assert frame.icp is None and "icp" not in frame.seconds and not frame.keyframe

    cam0 = _posed(cam, *poses[0])
    cam0 = slam._posed(np.asarray(cam0.rot, np.float64), np.asarray(cam0.tran, np.float64))
    seed = {k: v for k, v in opt.seed.items() if k != "color_dim"}
    params = gs_seed.seed_from_depth(targets[0][0], targets[0][1], cam0, color_dim=3, **seed)
    trainer = Trainer(params, [cam0], [targets[0][0]], opt.train, max_pairs=int(opt.max_pairs), depths=[targets[0][1]])
    for i in range(8):
        trainer.train_step(i, 0)
    tracker = Tracker(trainer.flat.params, cam0, opt.track, gpu)
    res = tracker.track(*targets[1])
    assert np.array_equal(frame.rot.view(np.uint64), res.rot.view(np.uint64))
    assert np.array_equal(frame.tran.view(np.uint64), res.tran.view(np.uint64))
    assert frame.tracked.losses == res.losses
