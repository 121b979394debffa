"""GPU tier of the off-centre principal point through tracking and the mapping loop (gs_track.Tracker, gs_slam.Slam).

The truth map, the arc and the helpers are those of tests/test_gpu_track.py and tests/test_gpu_slam.py (160 x 120, 20,000
Gaussians, 0.5 degrees and 0.02 per frame); the camera's principal point is moved by (+7.3, -4.6) pixels and every target is
rendered with that camera.  At this focal length (120 px) the offset is a 3.5-degree pointing error: seven times the motion the
Tracker is tested on -- which is what the control below relies on."""
import copy
import math

import numpy as np
import pytest
import torch

import pp_testutil as P
from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from test_gpu_slam import _colour_loss, _options, _posed, _poses
from track_ref import perturbed_start, pose_errors

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
OFF = P.OFFSETS[0]
_SCENE, _RUN = {}, {}


def _scene(gpu):
    """The truth map: (scene tensors, the offset camera, a renderer for the targets), built once."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        _SCENE["x"] = (to_torch(scene, gpu), P.offset_camera(cam, OFF),
                       FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False))
    return _SCENE["x"]


def _target(gpu, rot, tran):
    """(image, range map) of the truth scene seen from (rot, tran) through the offset camera."""
    params, cam, r = _scene(gpu)
    img, _, d, a = r.forward(*params, _posed(cam, rot, tran), training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
    return img.contiguous().clone(), rng.contiguous().clone()


# ------------------------------------------------------------------------------------------------------------ 12. tracking
@pytest.mark.parametrize("with_depth", [False, True])
def test_tracker_recovers_a_frame_of_an_offset_camera(gpu, with_depth):
    """tests/test_gpu_pose.py::test_pose_recovery's construction and criterion -- 0.5 degrees and 0.02 off, 300 iterations,
    both errors down to a tenth -- through the Tracker with the offset camera.  Control: the same target tracked with the
    offset dropped from the Tracker's camera does NOT meet the criterion (the pose would have to absorb the offset)."""
    from gs_track import TrackOptions, Tracker

    params, cam, _ = _scene(gpu)
    assert (cam.cx, cam.cy) == (80.0 + OFF[0], 60.0 + OFF[1])
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    assert abs(e_r0 - math.radians(0.5)) < 1e-4 and abs(e_t0 - 0.02) < 1e-9

    def run(camera):
        tr = Tracker(params, camera, TrackOptions(), gpu)
        res = tr.track(img, rng if with_depth else None, init=(R0, t0))
        assert res.iterations == 300
        return pose_errors(res.rot, res.tran, R_true, t_true)

    e_r, e_t = run(cam)
    centred = copy.copy(cam)
    centred.cx = centred.cy = None
    c_r, c_t = run(centred)
    print(f"PP tracker depth={with_depth}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}; "
          f"with the offset dropped: rot {c_r:.3e}, tran {c_t:.3e}")
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    assert not (c_r <= 0.1 * e_r0 and c_t <= 0.1 * e_t0), (c_r, c_t)


# ------------------------------------------------------------------------------------------------------------ 13. the loop
def _run(gpu):
    """The first four frames of tests/test_gpu_slam.py's arc through Slam with keyframe_every = 3 (keyframes 0 and 3), the
    camera's principal point moved by (+7.3, -4.6), observed as that file's _run observes its eight."""
    if "slam" in _RUN:
        return _RUN["slam"]
    from gs_slam import Slam

    _, cam, _ = _scene(gpu)
    poses = _poses(cam, 4)
    targets = [_target(gpu, R, t) for R, t in poses]
    slam = Slam(_posed(cam, *poses[0]), _options(keyframe_every=3), gpu)
    assert (slam.camera.cx, slam.camera.cy) == (cam.cx, cam.cy)
    seeded, rows = {}, []
    for f, ((R, t), (img, rng)) in enumerate(zip(poses, targets)):
        state = None
        if slam.trainer is not None:
            state = [slam.trainer.flat, slam.trainer.flat.flat_param.clone(), slam.trainer.optimizer.exp_avg.clone(),
                     slam.trainer.optimizer.exp_avg_sq.clone()]
        frame = slam.begin(img, rng)
        if frame.keyframe:
            kf = frame.window[0]
            seeded[kf] = _colour_loss(gpu, slam.params, slam.trainer.cameras[kf], slam.trainer.targets[kf],
                                      slam.opt.train.ssim_weight)
        assert slam.map(frame) is frame and frame.pending == 0
        unchanged = state is not None and slam.trainer.flat is state[0] and all(torch.equal(a, b) for a, b in zip(
            state[1:], [slam.trainer.flat.flat_param, slam.trainer.optimizer.exp_avg, slam.trainer.optimizer.exp_avg_sq]))
        rows.append(dict(frame=frame, err=pose_errors(frame.rot, frame.tran, R, t), unchanged=unchanged))
    final = {kf: _colour_loss(gpu, slam.params, slam.trainer.cameras[kf], slam.trainer.targets[kf],
                              slam.opt.train.ssim_weight) for kf in range(len(slam.keyframes))}
    motion = [None] + [pose_errors(*poses[k], *poses[k - 1]) for k in range(1, 4)]
    for f, row in enumerate(rows):
        mo = "-" if motion[f] is None else f"({motion[f][0]:.3e}, {motion[f][1]:.3e})"
        print(f"PP slam frame {f}: motion {mo} error ({row['err'][0]:.3e}, {row['err'][1]:.3e}) keyframe "
              f"{row['frame'].keyframe} added {row['frame'].added}")
    print("PP slam colour loss per keyframe, right after seeding -> at the end: "
          + ", ".join(f"{kf}: {seeded[kf]:.5f} -> {final[kf]:.5f}" for kf in sorted(final)))
    _RUN["slam"] = dict(slam=slam, rows=rows, seeded=seeded, final=final, motion=motion)
    return _RUN["slam"]


def test_the_loop_with_an_offset_camera(gpu):
    """That file's own criteria: from frame 2 on both pose errors are at most the motion since the frame before; each
    keyframe's colour loss ends below its seeded value; a frame that is no keyframe leaves the map and both Adam moments
    bitwise what they were.  Every camera the loop made -- the tracker's, the trainer's, the keyframe set's -- carries the
    principal point."""
    run = _run(gpu)
    slam, rows = run["slam"], run["rows"]
    assert [f for f, row in enumerate(rows) if row["frame"].keyframe] == [0, 3]
    for f in range(1, 4):
        assert abs(run["motion"][f][0] - math.radians(0.5)) < 1e-4 and abs(run["motion"][f][1] - 0.02) < 0.02 * 0.02
    for f in range(2, 4):
        err, mo = rows[f]["err"], run["motion"][f]
        assert err[0] <= mo[0] and err[1] <= mo[1], (f, err, mo)
    assert sorted(run["seeded"]) == sorted(run["final"]) == [0, 1]
    for kf in (0, 1):
        assert run["final"][kf] < run["seeded"][kf], (kf, run["seeded"][kf], run["final"][kf])
    for f, row in enumerate(rows):
        assert row["unchanged"] == (f not in (0, 3)), f
    _, cam, _ = _scene(gpu)
    for c in [slam.camera, slam.tracker.camera, *slam.trainer.cameras, *slam.keyframes.cameras]:
        assert (c.cx, c.cy) == (cam.cx, cam.cy)
    assert rows[3]["frame"].overlap.shape == (3,) and rows[3]["frame"].overlap[0] > 0.5 * rows[3]["frame"].overlap[1]
