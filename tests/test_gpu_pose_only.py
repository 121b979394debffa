"""GPU tier of the pose-only backward (gs_frame_backward_pose, include/gs_abi.h; FrameRenderer.backward_pose;
TrackOptions.pose_only): grad_rot, grad_tran and every partial row of the pose workspace bit for bit what
backward(..., grad_pose=...) leaves -- from the same gradient rows (part GS_BWD_GEOMETRY) and from a fresh forward (part 0) --,
nothing else written, and a Tracker with the option on returning the track of one with it off.  No tolerance anywhere."""
import copy

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import aux_case, general_camera, to_torch
from gs_track import TrackOptions, Tracker
from track_ref import perturbed_start

pytestmark = pytest.mark.gpu

GS_PB_BIG = 64  # frame_project_backward_body.inc: rows beyond which the whole workgroup sums an rgb Gaussian
RASTER, GEOMETRY = _lib.GS_BWD_RASTER, _lib.GS_BWD_GEOMETRY


def _nan_pose(gpu):
    return (torch.full((3, 3), float("nan"), device=gpu), torch.full((3,), float("nan"), device=gpu))


def _same_bits(a, b):
    """torch.equal on the bit patterns (an overflowed frame's rows may hold anything, NaNs included: equal all the same)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _partial_rows(r, n, aux):
    """A copy of the pose workspace's partial rows [(2 if aux else 1) ceil(n / 256), 12]: one row per workgroup of the
    projection's terms, then (aux) one per workgroup of the depth map's (gs_frame_layout.h: gs_frame_pose_carve)."""
    base = r._pose_ws.data_ptr()
    first = (base + 255) // 256 * 256 - base + 256
    rows = -(-n // 256) * (2 if aux else 1)
    return r._pose_ws[first:first + rows * 48].view(torch.float32).reshape(rows, 12).clone()


def _maps(gpu, H, W, kind, seed=5):
    """Seeded random dL/dimage (None for kind "aux_noimage") and, on aux frames, dL/ddepth / dL/dalpha."""
    gen = torch.Generator(gpu).manual_seed(seed)
    gimg = torch.randn(H, W, 3, device=gpu, generator=gen) if kind != "aux_noimage" else None
    gdep = torch.randn(H, W, device=gpu, generator=gen) * 0.1
    galp = torch.randn(H, W, device=gpu, generator=gen)
    return gimg, (dict(grad_depth=gdep, grad_alpha=galp) if kind != "plain" else {})


def _pose_pair(gpu, scene, cam, kind, r_kw=None, probe=None, max_pairs=1 << 20, auto_grow=True, whole_ws=False):
    """One forward and one backward(part=GS_BWD_RASTER); on those rows backward(part=GS_BWD_GEOMETRY, grad_pose) and
    backward_pose(part=GS_BWD_GEOMETRY) into NaN-filled destinations -- the second twice, over a pose workspace filled with 0xFF
    and with zeros --, the partial rows read back after each; then backward(part=0, grad_pose) against backward_pose(part=0),
    each on a fresh forward.  Everything must be equal bit for bit; the parameters and (whole_ws: the whole main workspace,
    the gradient rows among it) unchanged by backward_pose."""
    H, W = cam.height, cam.width
    aux = kind != "plain"
    params = to_torch(scene, gpu)
    n = params[0].shape[0]
    kept = [p.clone() for p in params]
    gimg, maps = _maps(gpu, H, W, kind)
    r = FrameRenderer(gpu, max_pairs=max_pairs, training=True, auto_grow=auto_grow, **(r_kw or {}))

    def forward():
        r.forward(*params, cam, aux=aux)
        if auto_grow:
            assert not r.last_frame_overflowed(wait=True)

    forward()
    if probe is not None:
        probe(r)
    out = tuple(torch.full_like(p, float("nan")) for p in params)
    r.backward(gimg, out=out, part=RASTER, **maps)
    ref = _nan_pose(gpu)
    r.backward(None, out=out, part=GEOMETRY, grad_pose=ref)
    rows_ref = _partial_rows(r, n, aux)
    geo_before = [t.clone() for t in out[:3]]
    ws_before = r._ws.clone() if whole_ws else None
    results = []
    for fill in (0xFF, 0x00, None):  # (None: whatever the call before left -- a plain repeat)
        if fill is not None:
            r._pose_ws.fill_(fill)
        got = _nan_pose(gpu)
        assert r.backward_pose(None, got, part=GEOMETRY) is got
        results.append((got, _partial_rows(r, n, aux)))
    if whole_ws:
        assert torch.equal(r._ws, ws_before), "backward_pose wrote into the frame's main workspace"
    # the gradient rows are what they were: the per-Gaussian geometry gradients come out of them again, bit for bit
    again = tuple(torch.full_like(p, float("nan")) for p in params)
    r.backward(None, out=again, part=GEOMETRY, grad_pose=_nan_pose(gpu))
    for a, b in zip(geo_before, again[:3]):
        assert _same_bits(a, b)
    # part 0, each on a fresh forward
    forward()
    ref0 = _nan_pose(gpu)
    r.backward(gimg, out=out, grad_pose=ref0, **maps)
    rows_ref0 = _partial_rows(r, n, aux)
    forward()
    r._pose_ws.fill_(0xFF)
    got0 = _nan_pose(gpu)
    r.backward_pose(gimg, got0, 0, **maps)
    results.append((got0, _partial_rows(r, n, aux)))
    for p, k in zip(params, kept):
        assert torch.equal(p, k)
    assert _same_bits(ref0[0], ref[0]) and _same_bits(ref0[1], ref[1]) and _same_bits(rows_ref0, rows_ref)  # (as before)
    for i, (got, rows) in enumerate(results):
        assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1]), (i, got, ref)
        assert _same_bits(rows, rows_ref), (i, (rows != rows_ref).nonzero().tolist()[:8], rows.shape)
    return ref, rows_ref


def _assert_live(ref, rows, aux):
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all() and torch.isfinite(rows).all()
    assert float(ref[0].abs().max()) > 0 and float(ref[1].abs().max()) > 0
    half = rows.shape[0] // 2 if aux else rows.shape[0]
    assert float(rows[:half].abs().max()) > 0
    if aux:
        assert float(rows[half:].abs().max()) > 0  # the depth map's rows


@pytest.mark.parametrize("n", [37, 6_000, 6_001])
@pytest.mark.parametrize("kind", ["plain", "aux", "aux_noimage"])
def test_pose_only_backward_equals_the_geometry_part(gpu, kind, n):
    """One partial wave; 6,000; 6,001 (N no multiple of 256) -- plain frames, aux frames with all three gradients, aux frames
    with dL/dimage = None.  At 37 the whole main workspace is compared across the call."""
    W, H = 160, 112
    ref, rows = _pose_pair(gpu, make_scene(n, W, H, seed=11), make_camera(W, H, yaw_deg=3.0), kind, whole_ws=n == 37)
    assert rows.shape[0] == -(-n // 256) * (1 if kind == "plain" else 2)
    _assert_live(ref, rows, kind != "plain")


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_pose_only_backward_with_workgroup_summed_and_culled_gaussians(gpu, kind):
    """Gaussians beyond GS_PB_BIG tiles (their rows summed by the whole workgroup: the depth float is then walked as the aux
    depth kernel walks it) and Gaussians the frustum culls (zeros in both sums) in one frame -- both asserted from the
    rectangle records."""
    W, H = 192, 128
    scene, cam = aux_case(8_000, W, H, seed=47, yaw=8.0, max_px_sigma=48.0)
    seen = []

    def probe(r):
        rc = r._rects()
        seen.append((int(((rc[:, 2] != 0) & (rc[:, 3] > GS_PB_BIG)).sum()), int((rc[:, 2] == 0).sum())))

    ref, rows = _pose_pair(gpu, scene, cam, kind, probe=probe)
    assert seen and seen[0][0] > 0 and seen[0][1] > 0, seen
    _assert_live(ref, rows, kind == "aux")


def _general_offcentre(W, H):
    cam = general_camera(W, H)
    cam.cx, cam.cy = W / 2 + 7.25, H / 2 - 4.5
    return cam


@pytest.mark.parametrize("case", ["general_camera", "exp_scales", "dist_listing"])
def test_pose_only_backward_other_cameras_and_settings(gpu, case):
    """One aux frame of 6,001 Gaussians each: fx != fy with an off-centre principal point; the exp scale activation; the
    "dist" listing (holes in the bounding square: the branch that gathers the projected centre from the record)."""
    W, H, n = 160, 112, 6_001
    scene, cam, r_kw = make_scene(n, W, H, seed=11), make_camera(W, H, yaw_deg=3.0), {}
    if case == "general_camera":
        cam = _general_offcentre(W, H)
    elif case == "exp_scales":
        scene.scale = np.log(np.abs(scene.scale) + 1e-4).astype(np.float32)
        r_kw = dict(scale_activation="exp")
    else:
        r_kw = dict(tile_culling_method="dist", tile_culling_dist_thresh=0.5)
    ref, rows = _pose_pair(gpu, scene, cam, "aux", r_kw=r_kw)
    _assert_live(ref, rows, True)


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_pose_only_backward_of_an_overflowed_frame_is_zero(gpu, kind):
    """A pair capacity far too small: the frame is rendered empty and the finalize kernel writes exact zeros, on both paths."""
    W, H = 128, 96
    ref, _ = _pose_pair(gpu, make_scene(4_000, W, H, seed=4), make_camera(W, H), kind, max_pairs=64, auto_grow=False)
    assert torch.equal(ref[0], torch.zeros(3, 3, device=gpu)) and torch.equal(ref[1], torch.zeros(3, device=gpu))


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_pose_only_backward_of_an_empty_frame_is_zero(gpu, kind):
    """N = 0: no kernel, no partial rows -- the pose workspace keeps the 0xFF it was filled with --; the pose gradient is
    written (zeros) all the same, by both parts."""
    cam, aux = make_camera(128, 96), kind == "aux"
    params = [torch.zeros(*s, device=gpu) for s in ((0, 3), (0, 4), (0, 3), (0,), (0, 3))]
    r = FrameRenderer(gpu, max_pairs=1 << 12, training=True, auto_grow=False)
    gimg, maps = _maps(gpu, cam.height, cam.width, kind)
    for part in (0, GEOMETRY):
        r.forward(*params, cam, aux=aux)
        got = _nan_pose(gpu)
        r._pose_frame(r._frame, got, 0)  # (allocates the pose workspace)
        r._pose_ws.fill_(0xFF)
        r.backward_pose(gimg, got, part, **(maps if part == 0 else {}))
        assert torch.equal(got[0], torch.zeros(3, 3, device=gpu)) and torch.equal(got[1], torch.zeros(3, device=gpu))
        assert bool((r._pose_ws == 0xFF).all())


def test_backward_pose_applies_the_checks_of_backward(gpu):
    W, H = 128, 96
    scene, cam = make_scene(500, W, H, seed=3), make_camera(W, H)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 16, training=True, auto_grow=True)
    gp = _nan_pose(gpu)
    with pytest.raises(RuntimeError, match=r"backward_pose\(\) needs a preceding forward\(training=True\)"):
        r.backward_pose(torch.ones(H, W, 3, device=gpu), gp)
    r.forward(*params, cam)
    with pytest.raises(RuntimeError, match="grad_depth / grad_alpha need"):
        r.backward_pose(torch.ones(H, W, 3, device=gpu), gp, grad_depth=torch.ones(H, W, device=gpu))
    with pytest.raises(RuntimeError, match="grad_image may be None"):
        r.backward_pose(None, gp)
    with pytest.raises(RuntimeError, match="grad_image must be float32"):
        r.backward_pose(torch.ones(H, W, device=gpu), gp)
    with pytest.raises(RuntimeError, match="grad_pose is written by"):
        r.backward_pose(torch.ones(H, W, 3, device=gpu), gp, part=RASTER)
    r.forward(*params, cam, aux=True)
    with pytest.raises(RuntimeError, match="grad_depth must be float32"):
        r.backward_pose(None, gp, grad_depth=torch.ones(W, H, device=gpu))
    assert all(torch.isnan(t).all() for t in gp)  # nothing was written by a refused call


# --------------------------------------------------------------------------------------------------------------- Tracker
W_, H_ = 160, 120
_SCENE = {}


def _scene(gpu):
    """The scene of tests/test_gpu_track.py, its target (image, range map) at the true pose and a start 0.5 degrees / 0.02 off."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False)
        img, _, d, a = r.forward(*params, copy.copy(cam), training=False, aux=True)
        rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
        start = perturbed_start(cam.rot.astype(np.float64), cam.tran.astype(np.float64))
        _SCENE["x"] = (params, cam, img.contiguous().clone(), rng.contiguous().clone(), start)
    return _SCENE["x"]


@pytest.mark.parametrize("variant", ["rgb", "rgbd", "median_gate", "pyramid"])
def test_tracker_with_pose_only_returns_the_same_track(gpu, variant):
    """12 iterations from the same start with the option off and on: pose, loss and every iteration's loss equal, the map
    untouched, and no per-Gaussian scratch on the pose-only side."""
    params, cam, img, rng, start = _scene(gpu)
    before = [p.clone() for p in params]
    kw = dict(iterations=12)
    if variant == "median_gate":
        kw["depth_gate_k"] = 10.0
    if variant == "pyramid":
        kw["pyramid"] = ((1, 4), (0, 4))
    res = {}
    for pose_only in (False, True):
        tr = Tracker(params, cam, TrackOptions(pose_only=pose_only, **kw), gpu)
        assert (tr._scratch is None) == pose_only
        res[pose_only] = tr.track(img, None if variant == "rgb" else rng, init=start)
        assert (tr._scratch is None) == pose_only
    a, b = res[False], res[True]
    assert a.iterations == b.iterations == (8 if variant == "pyramid" else 12)
    assert np.array_equal(a.rot, b.rot) and np.array_equal(a.tran, b.tran) and a.loss == b.loss
    assert len(a.losses) == len(b.losses) == a.iterations and all(x == y for x, y in zip(a.losses, b.losses))
    for p, k in zip(params, before):
        assert torch.equal(p, k)
