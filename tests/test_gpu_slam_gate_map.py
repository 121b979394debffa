"""GPU tier of SlamOptions.gate_map: two frames of the arc of tests/test_gpu_slam.py with keyframe_every = 1, the second
carrying the occluder rectangle of tests/test_gpu_track_gate.py, the tracker gated at k = 10 -- with the option the occluder is
neither seeded nor handed to the trainer, without it the loop is the one it was."""
import pytest
import torch

from test_gpu_slam import _frames, _posed, _scene
from test_gpu_track_gate import OCC_COLS, OCC_ROWS

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(gpu, gate_map):
    """First frame: step; second frame (occluded): begin only -- tracking, the gate and seeding are all in it.  Run once.

    The founding frame takes ``map_iterations`` = 120 steps, not ``map_iterations_first`` = 30: SlamOptions records that 30 (and
    60) steps leave a keyframe's colour loss above its seeded value and 120 bring it below, and in this two-frame run no later
    window ever revisits keyframe 0, so its founding steps are all the fit the map gets before it has to judge an occluder.
    The gate compares the frame with THAT map: where a 30-step map's expected depth is itself 30 - 50 % short of the truth (141
    pixels at depth edges inside the rectangle, measured) the halved range agrees with it and stays; after 120 steps 61 such
    pixels are left.  Measured range pixels removed: 5,650 of the 5,760 occluder pixels' worth with 30 steps (98.1 %, below the
    bound), 5,743 with 120."""
    if gate_map not in _RUNS:
        from gs_slam import Slam, SlamOptions
        from gs_track import TrackOptions

        _, cam, _ = _scene(gpu)
        poses, targets = _frames(gpu)
        img, rng = targets[1][0].clone(), targets[1][1].clone()
        img[OCC_ROWS, OCC_COLS] = torch.tensor([0.9, 0.1, 0.1], device=img.device)
        rng[OCC_ROWS, OCC_COLS] *= 0.5
        opt = SlamOptions(overlap_min=0.0, keyframe_every=1, track=TrackOptions(depth_gate_k=10.0), gate_map=gate_map)
        opt.map_iterations_first = opt.map_iterations
        slam = Slam(_posed(cam, *poses[0]), opt, gpu)
        slam.step(*targets[0])
        frame = slam.begin(img.contiguous(), rng.contiguous())
        _RUNS[gate_map] = (slam, frame, rng)
    return _RUNS[gate_map]


def test_gate_map_keeps_the_occluder_out_of_the_map(gpu):
    slam, frame, rng = _run(gpu, True)
    plain_slam, plain, _ = _run(gpu, False)
    occ = torch.zeros_like(rng, dtype=torch.bool)
    occ[OCC_ROWS, OCC_COLS] = True
    occ_measured = int((occ & (rng > 0)).sum())
    print(f"gate_map: gated {frame.gated} of {occ_measured} measured occluder pixels; seeded {frame.added} Gaussians against "
          f"{plain.added} without the option; tracked inliers {frame.tracked.inliers}")
    assert frame.keyframe and plain.keyframe and occ_measured > 5000
    assert frame.gated is not None and frame.gated[0] >= 0.99 * occ_measured
    assert frame.added <= plain.added / 10
    # the trainer's view 1 holds the gated range -- zeros exactly where GateMask.range has them -- and the weight; the keyframe
    # set keeps the raw range
    tr, gm = slam.trainer, slam.gate_mask
    assert len(tr.cameras) == 2 and torch.equal(tr.depths[1] == 0, gm.range == 0) and torch.equal(tr.depths[1], gm.range)
    assert tr.depths[1].data_ptr() != gm.range.data_ptr()  # (a copy: the next keyframe rewrites the GateMask's maps)
    assert tr.weights[0] is None and torch.equal(tr.weights[1], gm.weight)
    assert frame.gated == (int(((gm.range == 0) & (rng > 0)).sum()), int((gm.weight == 0).sum()))
    assert tr._weight_sums[1][0] == float((gm.weight != 0).sum())
    assert torch.equal(slam.keyframes.ranges[1], rng)
    # the mapping steps of the gated keyframe run (the weighted loss inside the fused step) and stay finite
    frame.pending = 4
    slam.map(frame)
    assert len(frame.map_losses) == 4 and all(v == v and v > 0 for v in frame.map_losses)


def test_without_the_option_the_loop_holds_no_gate(gpu):
    slam, frame, rng = _run(gpu, False)
    assert slam.gate_mask is None and slam._icp_renderer is None and frame.gated is None
    assert slam.trainer.weights is None and torch.equal(slam.trainer.depths[1], rng)
    assert frame.tracked.inliers is not None  # (the tracker itself was gated)
