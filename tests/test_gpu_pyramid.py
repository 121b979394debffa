"""GPU tier of coarse-to-fine tracking: gs_pyramid_down against the float32 restatement of tests/pyramid_ref.py bit for bit,
gs_pyramid.Pyramid, the level cameras together with the renderer, and gs_track.Tracker without and with a schedule of levels
(TrackOptions.pyramid).  include/gs_abi.h states the kernel's contract.

Shapes.  csrc/pyramid.hip: a lane makes one ITEM = four consecutive coarse pixels of one coarse row (fewer at the end of a row),
a coarse row has Q = ceil((W / 2) / 4) items, a workgroup is 256 consecutive items, one item per lane, NO grid cap (so no shape
"beyond the cap" exists).  16-byte accesses iff W % 8 == 0 (then W / 2 is a multiple of four and no row has a tail); every
other width is walked pixel by pixel, and only there can a row end in a tail of one to three pixels.
  (2, 2), (4, 6), (22, 36)      4-byte path, one workgroup or less; tails of 1, 3 and 2 pixels
  (10, 8), (6, 16), (30, 40)    16-byte path, one workgroup or less
  (120, 160)                    16-byte path, Q = 20: 1,200 items, five workgroups, shares end inside rows, the last partial
  (26, 320)                     16-byte path, chosen from the geometry: Q = 40 does not divide 256 -- every workgroup's share
                                ends inside a row -- and 13 x 40 = 520 items leave the third workgroup 8 of its 256 lanes
  (70, 84)                      the same on the 4-byte path: Q = 11 (a tail of two), 385 items, the second workgroup partial
(36 = W % 8 != 0 with W % 4 == 0: the fine rows are 16-byte aligned, the coarse rows are not -- the 4-byte path.)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pyramid_ref
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_pyramid import Pyramid, level_camera
from gs_scene import Scene, make_camera
from gs_testutil import to_torch
from gs_track import PoseAdam, TrackOptions, Tracker
from test_gpu_track import H_, W_, _scene, _target
from track_ref import perturbed_start, pose_errors

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (4, 6), (10, 8), (6, 16), (22, 36), (30, 40), (120, 160), (26, 320), (70, 84)]
SETTINGS = [(mv, er) for mv in (1, 2, 3, 4) for er in (-1.0, 0.0, 0.1)]


def _down(gpu, image, rng, H, W, min_valid, edge_rel):
    """One call into NaN-filled destinations -> (image_out, range_out or None) as numpy."""
    out = torch.full((H // 2, W // 2, 3), float("nan"), device=gpu)
    rout = torch.full((H // 2, W // 2), float("nan"), device=gpu) if rng is not None else None
    opts = _lib.GsPyramidOpts(min_valid, edge_rel)
    _lib.check(_lib.gs_pyramid_down(image.data_ptr(), rng.data_ptr() if rng is not None else None, H, W, C.byref(opts),
                                    out.data_ptr(), rout.data_ptr() if rng is not None else None,
                                    torch.cuda.current_stream().cuda_stream), "gs_pyramid_down")
    return out.cpu().numpy(), rout.cpu().numpy() if rng is not None else None


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("H,W", SHAPES)
def test_down_matches_the_restatement_bit_for_bit(gpu, H, W):
    """Colour and range, every min_valid with the edge test off, at 0 and at 0.1: equal to tests/pyramid_ref.py bit for bit,
    every element written (the destinations start as NaN; the inputs' colour holds none), two runs bitwise equal.  The range
    map mixes measured values with 0, negatives, NaN and +-inf; its first footprints hold n = 0..4 measured pixels and, from
    four rows on, one footprint with hi exactly fl(fl(1.1f) lo) -- measured at 0.1 -- beside one a float above -- not."""
    image, rng = pyramid_ref.inputs(H, W, seed=100 + H + W)
    ti, tr = torch.from_numpy(image).to(gpu), torch.from_numpy(rng).to(gpu)
    seen = set()
    for mv, er in SETTINGS:
        want_i, want_r = pyramid_ref.down(image, rng, mv, er)
        got_i, got_r = _down(gpu, ti, tr, H, W, mv, er)
        again_i, again_r = _down(gpu, ti, tr, H, W, mv, er)
        assert not np.isnan(got_i).any() and not np.isnan(got_r).any()  # everything written
        assert _same_bits(got_i, want_i), (mv, er, np.argwhere(got_i != want_i)[:4])
        assert _same_bits(got_r, want_r), (mv, er, np.argwhere(got_r != want_r)[:4])
        assert _same_bits(got_i, again_i) and _same_bits(got_r, again_r)
        seen.add((got_r > 0).tobytes())
        if H >= 4 and W >= 4 and mv <= 2:  # the two footprints on either side of the edge bound
            assert (got_r[1, 0] > 0) == (er != 0.0) and (got_r[1, 1] > 0) == (er < 0)
    if H * W >= 22 * 36:
        assert len(seen) >= 8  # the settings decide differently on these inputs
    # RGB only: the range pointers are NULL; the colour is the same
    got_i, got_r = _down(gpu, ti, None, H, W, 2, 0.1)
    assert got_r is None and _same_bits(got_i, pyramid_ref.down(image)[0])


def test_down_propagates_nan_colour_and_honours_the_stream(gpu):
    """No rule for NaN in the colour: it propagates to exactly the coarse pixels whose footprint holds one.  The launch goes to
    the stream it is given: issued on a side stream, visible after that stream is synchronised."""
    H, W = 30, 40
    image, rng = pyramid_ref.inputs(H, W, seed=3)
    image[7, 9, 1] = np.nan
    image[20, 33, :] = np.inf
    want_i, want_r = pyramid_ref.down(image, rng)
    s = torch.cuda.Stream(device=gpu)
    ti, tr = torch.from_numpy(image).to(gpu), torch.from_numpy(rng).to(gpu)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got_i, got_r = _down(gpu, ti, tr, H, W, 2, 0.1)
    assert _same_bits(got_i, want_i) and _same_bits(got_r, want_r)
    assert np.isnan(got_i[3, 4, 1]) and np.isnan(got_i).sum() == 1 and np.isinf(got_i[10, 16]).all()


# ------------------------------------------------------------------------------------------------------- 2. Pyramid.build
def test_pyramid_build(gpu):
    """Level 2 is the restatement applied twice, bitwise; entry 0 is the caller's tensor itself; a second build allocates
    nothing and returns the same buffers; RGB only: every range entry is None."""
    H, W = 44, 60  # 22 x 30 (4-byte path: 30 % 8 != 0 at level 1 -> 2), then 11 x 15
    image, rng = pyramid_ref.inputs(H, W, seed=9)
    ti, tr = torch.from_numpy(image).to(gpu), torch.from_numpy(rng).to(gpu)
    p = Pyramid(H, W, 2, gpu)
    images, ranges = p.build(ti, tr)
    assert images[0] is ti and ranges[0] is tr and len(images) == len(ranges) == 3
    want = pyramid_ref.level(image, rng, 2)
    mid = pyramid_ref.level(image, rng, 1)
    assert _same_bits(images[1].cpu().numpy(), mid[0]) and _same_bits(ranges[1].cpu().numpy(), mid[1])
    assert _same_bits(images[2].cpu().numpy(), want[0]) and _same_bits(ranges[2].cpu().numpy(), want[1])
    assert tuple(images[2].shape) == (11, 15, 3) and (want[1] > 0).any() and (want[1] == 0).any()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    images2, ranges2 = p.build(ti, tr)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before
    assert all(a is b for a, b in zip(images + ranges, images2 + ranges2))
    images3, ranges3 = p.build(ti)
    assert ranges3 == [None, None, None] and _same_bits(images3[2].cpu().numpy(), want[0])
    other = Pyramid(H, W, 2, gpu, min_valid=4, edge_rel=-1.0).build(ti, tr)[1][2].cpu().numpy()
    assert _same_bits(other, pyramid_ref.level(image, rng, 2, 4, -1.0)[1]) and not _same_bits(other, want[1])
    flat = Pyramid(H, W, 0, gpu).build(ti, tr)
    assert len(flat[0]) == len(flat[1]) == 1 and flat[0][0] is ti and flat[1][0] is tr
    with pytest.raises(RuntimeError, match="image must be a contiguous float32 HIP tensor of shape \\[44, 60, 3\\]"):
        p.build(ti[:, :, :2])
    with pytest.raises(RuntimeError, match="range_map must be"):
        p.build(ti, tr.double())


# ------------------------------------------------------------------------------------- 3. level camera and renderer together
def test_level_cameras_render_the_same_place(gpu):
    """One isotropic rgb Gaussian of sigma = 8 fine pixels inside a 60 x 44 frame whose principal point is off-centre.  The
    alpha-weighted centroid sum A (i + 1/2, j + 1/2) / sum A of the frame rendered under level_camera(cam, l), times 2^l, is
    the level-0 centroid within 0.1 fine pixel for l = 1 (30 x 22) and l = 2 (15 x 11: an odd size, half a coarse pixel off
    that level's own centre).  The tolerance: a Gaussian two or more coarse pixels wide is sampled without visible error
    (the midpoint sums of the same window differ by a few hundredths of a pixel at most), the renderer's cut-off is symmetric
    -- while any half-pixel convention error is at least 1 fine pixel at level 1 and 2 at level 2."""
    W, H, z, sigma_px = 60, 44, 3.0, 8.0
    cam = make_camera(W, H)
    cam.cx, cam.cy = 33.25, 20.5
    s = sigma_px * z / cam.focal_x
    u0, v0 = 31.3, 21.6  # where the Gaussian's centre projects, in fine pixel coordinates
    pos = np.array([[(u0 - cam.cx) / cam.focal_x * z, (v0 - cam.cy) / cam.focal_y * z, z]], np.float32)
    scene = Scene(pos, np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), np.full((1, 3), s - 1e-4, np.float32),
                  np.array([1.5], np.float32), np.zeros((1, 3), np.float32))
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=4096, training=False, auto_grow=True, occlusion_cull=False)
    cents = []
    for l in (0, 1, 2):
        c = level_camera(cam, l)
        with torch.no_grad():
            _, _, alpha = r.render_aux(*params, c)
        a = alpha.cpu().numpy().astype(np.float64)
        assert a.shape == (H >> l, W >> l) and a.max() > 0.5
        jj, ii = np.meshgrid(np.arange(H >> l) + 0.5, np.arange(W >> l) + 0.5, indexing="ij")
        cents.append((float((a * ii).sum() / a.sum()) * 2 ** l, float((a * jj).sum() / a.sum()) * 2 ** l))
    print(f"level-camera centroids (fine pixels): {cents}; the centre projects to ({u0}, {v0})")
    assert abs(cents[0][0] - u0) <= 0.5 and abs(cents[0][1] - v0) <= 0.5  # (level 0 itself: tests/test_gpu_pp.py pins it)
    for l in (1, 2):
        assert abs(cents[l][0] - cents[0][0]) <= 0.1 and abs(cents[l][1] - cents[0][1]) <= 0.1, (l, cents)


# ----------------------------------------------------------------------------------------------- 4. Tracker, no schedule
def test_tracker_without_a_schedule_is_the_loop_it_was(gpu):
    """TrackOptions() and TrackOptions(pyramid=((0, 300),)) return poses and losses bitwise equal to the loop assembled here
    from Tracker.iteration and PoseAdam -- the statement of track() before schedules existed.  Either holds one renderer; the
    default one holds no Pyramid and no per-level table."""
    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    o = TrackOptions()
    tr = Tracker(params, cam, o, gpu)
    tr0 = Tracker(params, cam, TrackOptions(pyramid=((0, 300),)), gpu)
    for x in (tr, tr0):  # one renderer each
        assert [type(v) for v in vars(x).values()].count(FrameRenderer) == 1
    assert tr._levels is None and tr._pyramid is None and tr._stages is None
    assert list(tr0._levels) == [0] and tr0._levels[0][0] is tr0.renderer and tr0._levels[0][2] is cam
    # the loop, by hand
    R, t = R0.copy(), t0.copy()
    adam = PoseAdam(R, t, o.lr_rot, o.lr_tran, o.betas, o.eps)
    best, losses = (math.inf, R, t), []
    hand = Tracker(params, cam, o, gpu)
    for k in range(300):
        h = hand.iteration(R, t, img, rng).numpy().astype(np.float64)
        losses.append(float(h[12]))
        if losses[-1] < best[0]:
            best = (losses[-1], R, t)
        R, t = adam.step(h[0:9], h[9:12], o.lr_final ** (k / 300))
    res, res0 = tr.track(img, rng, init=(R0, t0)), tr0.track(img, rng, init=(R0, t0))
    for got in (res, res0):
        assert got.losses == losses and got.loss == best[0] and got.iterations == 300
        assert got.rot.tobytes() == best[1].tobytes() and got.tran.tobytes() == best[2].tobytes()
    assert res.levels is None and res0.levels == [(0, 0, 300)]
    assert best[0] < losses[0]
    with pytest.raises(ValueError, match="no schedule"):
        tr.iteration(R0, t0, img, rng, level=1)
    with pytest.raises(ValueError, match="not in this Tracker's schedule"):
        tr0.iteration(R0, t0, img, rng, level=1)


# --------------------------------------------------------------------------------------------- 5. Tracker, with a schedule
SCHEDULE = ((2, 100), (1, 100), (0, 100))  # level-0-equivalent work 100 / 16 + 100 / 4 + 100 = 131.25 <= 150


@pytest.mark.parametrize("with_depth", [False, True])
def test_tracker_with_a_schedule_recovers_a_single_frame(gpu, with_depth):
    """The case and criterion of tests/test_gpu_track.py::test_tracker_recovers_a_single_frame (0.5 degrees and 0.02 off, both
    errors down to a tenth) under the schedule ((2, 100), (1, 100), (0, 100)): 40 x 30, 80 x 60, then 160 x 120."""
    params, cam, _ = _scene(gpu)
    before = [p.clone() for p in params]
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(pyramid=SCHEDULE), gpu)
    assert sorted(tr._levels) == [0, 1, 2] and len({id(v[0]) for v in tr._levels.values()}) == 3  # a renderer per level
    res = tr.track(img, rng if with_depth else None, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    print(f"tracker schedule {SCHEDULE} depth={with_depth}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, "
          f"losses at the stage starts {[round(res.losses[k], 5) for k in (0, 100, 200)]}, ends "
          f"{[round(res.losses[k], 6) for k in (99, 199, 299)]}, returned {res.loss:.6f}")
    assert abs(e_r0 - math.radians(0.5)) < 1e-4 and abs(e_t0 - 0.02) < 1e-9
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    for a, b in zip(before, params):
        assert torch.equal(a, b) and a.grad is None and b.grad is None  # the map is bitwise unchanged
    assert np.abs(res.rot @ res.rot.T - np.eye(3)).max() <= 1e-6
    assert res.iterations == 300 == len(res.losses) and res.loss == min(res.losses[200:])
    assert res.levels == [(2, 0, 100), (1, 100, 100), (0, 200, 100)]
    assert res.inliers is None and res.medians is None
    again = float(tr.iteration(res.rot, res.tran, img, rng if with_depth else None, level=0)[12])
    assert again == res.loss  # the loss that came back belongs to the pose that came back, at full resolution


def test_tracker_with_a_schedule_and_the_median_gate(gpu):
    """The same schedule with depth_gate_k = 10: a gated loss object per level, and the inliers / medians that come back are
    those of the returned pose's iteration -- a level-0 one."""
    from gs_train import GatedTrackLoss

    params, cam, _ = _scene(gpu)
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, rng = _target(gpu, R_true, t_true)
    R0, t0 = perturbed_start(R_true, t_true)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(pyramid=SCHEDULE, depth_gate_k=10.0), gpu)
    assert all(type(v[1]) is GatedTrackLoss and (v[1].H, v[1].W) == (H_ >> l, W_ >> l) for l, v in tr._levels.items())
    res = tr.track(img, rng, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    print(f"tracker schedule {SCHEDULE} gated: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, inliers "
          f"{res.inliers}, medians {res.medians}")
    assert res.loss == min(res.losses[200:]) and res.levels == [(2, 0, 100), (1, 100, 100), (0, 200, 100)]
    again = tr.iteration(res.rot, res.tran, img, rng, level=0)
    assert again.numel() == 20 and float(again[12]) == res.loss
    assert res.inliers == (int(again[15]), int(again[19]), int(again[16])) and res.medians == (float(again[17]), float(again[18]))
    # a level-0 iteration: n_d counts full-resolution pixels -- more than the 80 x 60 of level 1 holds
    assert (W_ >> 1) * (H_ >> 1) < res.inliers[1] <= W_ * H_ and 0 < res.inliers[0] <= res.inliers[1]
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
