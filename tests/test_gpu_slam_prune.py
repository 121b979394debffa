"""GPU tier of the map edits inside the mapping loop (gs_slam.Slam with ``carry_optimizer`` and ``prune_every``): a four-frame
prefix of the arc of tests/test_gpu_slam.py (160 x 120, the 20,000-Gaussian truth scene, 0.5 degrees and 0.02 per frame; its
helpers are restated here), keyframes at frames 0 and 3, a few dozen mapping steps each.  No assertion that carrying the
optimizer state improves the losses: profiles/slam_carry.txt reports what it did on the eight-frame arc."""
import copy
import math

import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from track_ref import so3_exp_series

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
N_FRAMES = 4
MAP_FIRST, MAP_LATER = 30, 24
# Seeds start at opacity 0.9 (logit 2.2).  The opacity rate is 0.03 per step behind a five-step warm-up, and Adam moves a
# parameter whose gradient keeps its sign by about the rate per step: thirty steps can take a logit down by ~0.8, to 0.80.
# A floor of 0.85 (logit 1.73) therefore removes the seeds training pushed down hardest and keeps the ones it left alone.
# (Measured on an MI355X: 12 of 19,200 behind keyframe 0's steps, 376 behind keyframe 1's.  Not a floor to map with: on the
# eight-frame arc it takes a third of the map, profiles/slam_carry.txt.)
PRUNE_OPA_MIN = 0.85


def _posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def _frames(gpu):
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
    for _ in range(N_FRAMES - 1):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    targets = []
    for R, t in poses:
        img, _, d, a = r.forward(*params, _posed(cam, R, t), training=False, aux=True)
        rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
        targets.append((img.contiguous().clone(), rng.contiguous().clone()))
    return cam, poses, targets


def test_the_loop_prunes_and_never_resets_adam(gpu):
    from gs_slam import Slam, SlamOptions

    cam, poses, targets = _frames(gpu)
    opts = SlamOptions(overlap_min=0.0, keyframe_every=3, map_iterations_first=MAP_FIRST, map_iterations=MAP_LATER,
                       carry_optimizer=True, prune_every=1, prune_opa_min=PRUNE_OPA_MIN)
    slam = Slam(_posed(cam, *poses[0]), opts, gpu)
    rows = []
    for f, (img, rng) in enumerate(targets):
        tr = slam.trainer
        state = None
        if tr is not None:
            state = [tr.flat, tr.optimizer, tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(),
                     tr.optimizer.exp_avg_sq.clone(), tr.optimizer.step_count]
        frame = slam.begin(img, rng)
        n_seeded = slam.trainer.n_gaussians
        assert slam.map(frame) is frame
        tr = slam.trainer
        assert frame.pruned == n_seeded - tr.n_gaussians  # the drop in n_gaussians
        if frame.keyframe:
            assert frame.pruned >= 0 and "prune" in frame.seconds
        else:  # a frame that is no keyframe leaves the parameters and the moments alone, bit for bit
            assert frame.pruned == 0 and "prune" not in frame.seconds
            assert tr.flat is state[0] and tr.optimizer is state[1] and tr.optimizer.step_count == state[5]
            for a, b in zip(state[2:5], [tr.flat.flat_param, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq]):
                assert torch.equal(a, b)
        # the tracker reads the trainer's CURRENT tensors (after a prune the old ones are another size)
        assert all(a.data_ptr() == b.data_ptr() and a.shape == b.shape
                   for a, b in zip(slam.tracker.params, tr.flat.params))
        rows.append(frame)
        print(f"  frame {f}: keyframe {frame.keyframe} added {frame.added} pruned {frame.pruned} Gaussians {tr.n_gaussians} "
              f"step count {tr.optimizer.step_count}")
    assert [fr.keyframe for fr in rows] == [True, False, False, True]
    assert rows[0].pruned > 0 and rows[3].added > 0  # (the floor takes something: the test means something)
    # the optimizer was never reset: its step count is the number of mapping steps taken
    assert slam.i_iter == MAP_FIRST + MAP_LATER == slam.trainer.optimizer.step_count
    assert all(math.isfinite(v) for fr in rows for v in fr.map_losses)
    assert slam.trainer.optimizer.exp_avg.abs().max() > 0


def test_the_options_are_off_by_default(gpu):
    """With the defaults the loop rebinds as it always did: a keyframe's seeding starts a fresh optimizer (the step count
    restarts) and nothing is pruned."""
    from gs_slam import Slam, SlamOptions

    cam, poses, targets = _frames(gpu)
    slam = Slam(_posed(cam, *poses[0]), SlamOptions(overlap_min=0.0, keyframe_every=3, map_iterations_first=6,
                                                   map_iterations=4), gpu)
    frames = [slam.step(*t) for t in targets]
    assert [fr.pruned for fr in frames] == [0, 0, 0, 0] and all("prune" not in fr.seconds for fr in frames)
    assert frames[3].keyframe and frames[3].added > 0 and slam.trainer.optimizer.step_count == 4 and slam.i_iter == 10
