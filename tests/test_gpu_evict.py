"""GPU tier of keyframe eviction (gs_train.Trainer.remove_view, gs_slam.SlamOptions.max_keyframes): a view removed from a
running fit against the fit built without it, bit for bit, and the capped loop on the eight-frame arc of
tests/test_gpu_slam.py (160 x 120, 20,000 Gaussians, 0.5 degrees and 0.02 per frame; that file's helpers are restated here) --
which keyframe goes is decided on the CPU by tests/redundancy_ref.py and gs_slam.select_eviction from a snapshot of the
keyframe set, every time.  Few steps per frame: nothing here asserts a pose or a loss."""
import copy
import math

import numpy as np
import pytest
import torch

import redundancy_ref as RR
from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from track_ref import so3_exp_series

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


# ---------------------------------------------------------------------------------------------- 1. Trainer.remove_view
def test_remove_view_leaves_the_fit_the_constructor_would_have_built(gpu):
    """Views [A, B, C] at construction, one step on A, remove_view(1): the next six steps alternating over the remaining views
    leave the parameters and both Adam moments equal, bit for bit, to those of a trainer built on [A, C] that took the same
    steps; remove_view itself changes none of them; the per-view keys shift; the two refusals raise."""
    from gs_seed import seed_from_depth
    from gs_train import TrainOptions, Trainer

    _, cam, _ = _scene(gpu)
    poses, targets = _frames(gpu)
    pick = (0, 3, 5)
    cams = [_posed(cam, *poses[f]) for f in pick]
    images, ranges = [targets[f][0] for f in pick], [targets[f][1] for f in pick]
    start = seed_from_depth(images[0], ranges[0], cams[0], stride=2)
    opt = TrainOptions(n_iters_warmup=2, depth_weight=0.2)

    def state(tr):
        return [tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone()]

    def keep(lst):
        return [lst[0], lst[2]]

    three = Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 21, depths=ranges)
    two = Trainer([t.clone() for t in start], keep(cams), keep(images), opt, max_pairs=1 << 21, depths=keep(ranges))
    three.train_step(0, 0)
    two.train_step(0, 0)
    before, flat, optimizer, steps = state(three), three.flat, three.optimizer, three.optimizer.step_count
    assert three._views_checked == {0}
    three._views_checked.add(2)  # (as if view C had been rendered: its key must follow it down)
    three.remove_view(1)
    assert three.flat is flat and three.optimizer is optimizer and three.optimizer.step_count == steps
    assert all(torch.equal(a, b) for a, b in zip(before, state(three)))
    assert len(three.cameras) == len(three.targets) == len(three.depths) == len(three._depth_inv_n) == 2
    assert three.cameras[1] is cams[2] and three.targets[1] is images[2] and torch.equal(three.depths[1], two.depths[1])
    assert three._depth_inv_n == two._depth_inv_n and three._views_checked == {0, 1}
    three._views_checked.discard(1)
    for i in range(1, 7):
        two.train_step(i, i % 2)
        three.train_step(i, i % 2)
    for a, b in zip(state(two), state(three)):
        assert torch.equal(a, b)
    assert not torch.equal(before[0], state(three)[0])  # (the steps moved the parameters: the comparison means something)
    # the refusals, and the keys of free poses and weights
    with pytest.raises(IndexError):
        three.remove_view(2)
    three.remove_view(0)
    assert len(three.cameras) == 1 and three.cameras[0] is cams[2]
    with pytest.raises(ValueError, match="without a view"):
        three.remove_view(0)
    assert len(three.cameras) == 1
    wmap = torch.ones((H_, W_), device=gpu)
    other = Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 21, depths=ranges,
                    weights=[None, None, wmap])
    other.free_pose(1, 2e-4, 2e-4)
    other.free_pose(2, 2e-4, 2e-4)
    with pytest.raises(RuntimeError, match="free pose"):
        other.remove_view(1)
    assert len(other.cameras) == 3 and sorted(other._free) == [1, 2]
    free2 = other._free[2]
    other.fix_pose(1)
    other.remove_view(1)
    assert sorted(other._free) == [1] and other._free[1] is free2
    assert other.weights[0] is None and torch.equal(other.weights[1], wmap)
    assert len(other.weights) == len(other._weight_sums) == len(other.cameras) == 2 and other._weight_sums[1][0] == H_ * W_
    other.fix_pose(1)


# ------------------------------------------------------------------------------------------------------- 2. the loop
def _options(**kw):
    from gs_slam import SlamOptions
    from gs_track import TrackOptions

    return SlamOptions(track=TrackOptions(iterations=40), map_iterations=10, map_iterations_first=10, overlap_min=0.0, **kw)


def _run(gpu, name, n_frames=N_FRAMES, **kw):
    """The arc through a capped Slam, observed: per frame the SlamFrame, a snapshot of the keyframe set taken BEFORE it, and
    the lengths of the set and the trainer after it.  Run once per configuration."""
    if name in _RUN:
        return _RUN[name]
    from gs_slam import Slam

    _, cam, _ = _scene(gpu)
    poses, targets = _frames(gpu)
    slam = Slam(_posed(cam, *poses[0]), _options(**kw), gpu)
    rows = []
    for (img, rng) in targets[:n_frames]:
        ks = slam.keyframes
        snap = dict(cameras=list(ks.cameras), ranges=list(ks.ranges), ids=list(ks.ids))
        frame = slam.step(img, rng)
        rows.append(dict(frame=frame, snap=snap, n_keyframes=len(slam.keyframes), n_views=len(slam.trainer.cameras),
                         ids=list(slam.keyframes.ids)))
    _RUN[name] = dict(slam=slam, rows=rows)
    print(f"{name}: " + ", ".join(f"frame {f}: keyframe {r['frame'].keyframe} evicted {r['frame'].evicted} ids {r['ids']}"
                                  for f, r in enumerate(rows)))
    return _RUN[name]


def _decided_on_the_cpu(slam, snap):
    """The id select_eviction picks from hist_f32 of a snapshot of the keyframe set, with the loop's options."""
    from gs_slam import select_eviction

    o = slam.opt
    stride = o.evict_stride if o.evict_stride is not None else o.stride
    n = len(snap["cameras"])
    hists = np.stack([RR.hist_f32(snap["ranges"][k].cpu().numpy(), snap["cameras"][k], snap["cameras"], k, stride, slam.near,
                                  o.border) for k in range(n)])
    assert (hists[:, 8] > 0).all()
    pos = select_eviction(hists, o.evict_seen_by, protected=(0, n - 1))
    return snap["ids"][pos], hists


def test_cap_of_three_leaves_one_candidate(gpu):
    """keyframe_every = 2, max_keyframes = 3: keyframes at frames 0, 2, 4, 6; at frame 6 the set is full, positions 0 and 2 are
    protected, position 1 goes."""
    run = _run(gpu, "cap 3", keyframe_every=2, max_keyframes=3)
    slam, rows = run["slam"], run["rows"]
    assert [f for f, r in enumerate(rows) if r["frame"].keyframe] == [0, 2, 4, 6]
    for f, r in enumerate(rows[:6]):
        assert r["frame"].evicted is None and "evict" not in r["frame"].seconds, f
    last = rows[6]["frame"]
    assert last.evicted == 1 and last.seconds["evict"] > 0 and rows[7]["frame"].evicted is None
    assert len(slam.keyframes) == 3 and slam.keyframes.ids == [0, 2, 3] and len(slam.trainer.cameras) == 3
    assert len(slam.trainer.targets) == len(slam.trainer.depths) == len(slam.trainer._depth_inv_n) == 3
    assert 1 not in last.window_ids and last.window_ids[0] == 3 and last.window[0] == 2
    assert last.window_ids == [slam.keyframes.ids[v] for v in last.window] and set(last.window_ids) <= {0, 2, 3}
    assert last.overlap.shape == (3 + 2,)  # the counts as computed, before the removal
    assert len(last.map_losses) == slam.opt.map_iterations and all(math.isfinite(v) for v in last.map_losses)
    assert _decided_on_the_cpu(slam, rows[6]["snap"])[0] == 1
    for r in rows:
        assert r["n_keyframes"] == r["n_views"] <= 3
        fr = r["frame"]
        assert fr.window_ids == ([r["ids"][v] for v in fr.window] if fr.keyframe else [])
    # the views of the trainer are the keyframes that remain, in order
    for a, b in zip(slam.trainer.cameras, slam.keyframes.cameras):
        assert np.array_equal(a.rot, b.rot) and np.array_equal(a.tran, b.tran)
    assert all(a is b for a, b in zip(slam.trainer.targets, slam.keyframes.images))


def test_every_eviction_is_the_one_decided_on_the_cpu(gpu):
    """keyframe_every = 1, max_keyframes = 4: from the fifth keyframe on every frame evicts, and two positions are candidates.
    The evicted id equals select_eviction applied to hist_f32 of the keyframe set as it was before the frame."""
    from gs_slam import select_keyframes

    run = _run(gpu, "cap 4", keyframe_every=1, max_keyframes=4)
    slam, rows = run["slam"], run["rows"]
    assert all(r["frame"].keyframe for r in rows)
    evicted = []
    for f, r in enumerate(rows):
        fr = r["frame"]
        assert r["n_keyframes"] == r["n_views"] == min(f + 1, 4), f
        if f < 4:
            assert fr.evicted is None
            continue
        want, hists = _decided_on_the_cpu(slam, r["snap"])
        assert fr.evicted == want, (f, fr.evicted, want, hists)
        assert fr.evicted != 0 and fr.evicted != r["snap"]["ids"][-1] and fr.evicted in r["snap"]["ids"]
        assert fr.evicted not in r["ids"] and r["ids"][0] == 0 and r["ids"][-1] == f  # the new keyframe's id: its frame
        assert fr.window_ids[0] == f and fr.evicted not in fr.window_ids
        # the window: chosen from the counts without the evicted keyframe's column
        gone = r["snap"]["ids"].index(fr.evicted)
        counts = np.delete(fr.overlap[:4], gone)
        assert fr.window[1:] == select_keyframes(counts, int(fr.overlap[4]), slam.opt.window - 1, slam.opt.min_share)
        evicted.append(fr.evicted)
    assert len(evicted) == 4 and len(set(evicted)) == 4
    assert slam.keyframes.n_added == N_FRAMES and len(slam.keyframes) == 4


def test_no_cap_no_eviction(gpu):
    """max_keyframes = 0 (the default): no frame evicts, no redundancy count is issued, ids are positions."""
    import gs_slam

    calls = []
    original = gs_slam.view_redundancy
    gs_slam.view_redundancy = lambda *a, **kw: calls.append(1) or original(*a, **kw)
    try:
        run = _run(gpu, "no cap", n_frames=5, keyframe_every=2)
    finally:
        gs_slam.view_redundancy = original
    assert run["slam"].opt.max_keyframes == 0 and not calls
    for r in run["rows"]:
        fr = r["frame"]
        assert fr.evicted is None and "evict" not in fr.seconds and fr.window_ids == fr.window
        assert r["ids"] == list(range(r["n_keyframes"]))
    assert [r["frame"].keyframe for r in run["rows"]] == [True, False, True, False, True]
