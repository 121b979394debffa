"""GPU tier of the scene pack (GS_FRAME_SCENE_PACK, include/gs_abi.h): from its second consecutive inference frame of the same
tensors on, a renderer projects from a cached, camera-independent pack (cull_project.hip: scene_pack_build_kernel and the PACKED
variants of frame_project_count_kernel / frame_project_cull_count_kernel) instead of the raw parameter arrays.

The contract is bit-for-bit equality: every comparison below is `torch.equal` against a `FrameRenderer(scene_pack=False, ...)`
on the same inputs (the oracle is reached through the existing tests, most of which now run packed from their second frame).

Shapes: 140 k Gaussians at 320 x 240 is the smallest size at which the strip variant is the product's own path (183 slices of
768, a ragged last slice); 800 k at 640 x 384 gives slices of 3,328, the smallest that take the unrolled-by-three phase-A loop
round again, with a partial last slice."""
import functools

import numpy as np
import pytest
import torch

from gs_dp import FlatGaussianParams
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import to_torch
from gs_train import FusedAdam, TrainOptions, base_lrs

pytestmark = pytest.mark.gpu

N, W, H = 140_000, 320, 240
MAX_PAIRS = 1 << 20


@functools.lru_cache(maxsize=None)
def _opaque_arrays(n=N, w=W, h=H, seed=21, use_sh=False):
    scene = make_scene(n, w, h, seed=seed, use_sh=use_sh, sh_degree=2)
    scene.opa += 3.0  # opaque: every tile's pixels stop long before the end of its list
    return scene


def _opaque(gpu, n=N, w=W, h=H, seed=21, use_sh=False, act="abs"):
    """Fresh device tensors of the (cached, never modified) opaque scene."""
    scene = _opaque_arrays(n, w, h, seed, use_sh)
    params = to_torch(scene, gpu)
    if act == "exp":  # (scales log-transformed: the same activated scales through exp)
        params[2] = torch.from_numpy(np.log(scene.scale)).to(gpu)
    return params


def _bits(img):
    return img.contiguous().view(torch.int32)


def _same_frame(a, b):
    """Image bit for bit, NaN pixels included."""
    return torch.equal(_bits(a), _bits(b))


def _fresh_raw(gpu, params, cam, **kw):
    r = FrameRenderer(gpu, scene_pack=False, occlusion_cull=False, **dict(dict(max_pairs=MAX_PAIRS), **kw))
    return r.forward(*params, cam, training=False)[0]


# ------------------------------------------------------------------------------------------ the pack against the records
@pytest.mark.parametrize("color_dim", [3, 27])
@pytest.mark.parametrize("method", ["prob2", "prob", "dist"])
@pytest.mark.parametrize("act", ["abs", "exp"])
def test_packed_frames_write_the_raw_frames_records(gpu, act, method, color_dim):
    """Unculled frames: the first frame of a key renders raw, the second builds the pack and reads it, the third re-uses it;
    image, counters, rectangle records and the per-Gaussian 64-byte records equal the raw renderer's."""
    params = _opaque(gpu, use_sh=color_dim != 3, act=act)
    assert params[4].shape[1] == color_dim
    cam = make_camera(W, H)
    kw = dict(max_pairs=1 << 21, occlusion_cull=False, scale_activation=act, tile_culling_method=method)
    r, raw = FrameRenderer(gpu, **kw), FrameRenderer(gpu, scene_pack=False, **kw)
    ref, _ = raw.forward(*params, cam)
    assert not raw.scene_pack_active() and raw.binning_variant() == "strip"
    want, want_st, want_rects = raw.debug_views(), raw.stats(), raw._rects().clone()
    want = {k: v.clone() for k, v in want.items()}
    assert want_st.overflow == 0 and want_st.pairs > 0 and 0 < want_st.visible < N
    for k in range(3):
        img, _ = r.forward(*params, cam)
        assert r.scene_pack_active() == (k >= 1), k
        st = r.stats()
        assert _same_frame(img, ref), k
        assert (st.visible, st.pairs, st.overflow) == (want_st.visible, want_st.pairs, 0), (k, st, want_st)
        assert torch.equal(r._rects(), want_rects), k
        got = r.debug_views()
        assert set(got) == set(want)
        for name in want:
            assert torch.equal(_bits(got[name]) if got[name].dtype == torch.float32 else got[name],
                               _bits(want[name]) if want[name].dtype == torch.float32 else want[name]), (k, name)
    assert raw.forward(*params, cam) is not None and not raw.scene_pack_active()  # scene_pack=False: never


# ------------------------------------------------------------------------------------------ culled, static pose
@pytest.mark.parametrize("w,h", [(320, 240), (300, 232)])
def test_culled_static_pose(gpu, w, h):
    """Occlusion-culled frames at rest (300 x 232: ragged strips, a height that is no multiple of 16): frames 2 - 5 are culled,
    packed and do not fall back; the image is the unculled raw renderer's, the emitted pairs and the visible count those of
    the culled raw renderer (the emitted lists do not depend on the Gaussian-level occlusion test)."""
    params = _opaque(gpu, N, w, h)
    cam = make_camera(w, h)
    kw = dict(max_pairs=MAX_PAIRS, auto_grow=False)
    r = FrameRenderer(gpu, **kw)
    cull_raw = FrameRenderer(gpu, scene_pack=False, **kw)
    off = FrameRenderer(gpu, scene_pack=False, occlusion_cull=False, **kw)
    ref, _ = off.forward(*params, cam)
    for k in range(5):
        r._cull_off_until = cull_raw._cull_off_until = 0  # (the adaptive policy kept out of the way)
        img, _ = r.forward(*params, cam)
        st = r.stats()
        other, _ = cull_raw.forward(*params, cam)
        st_raw = cull_raw.stats()
        assert _same_frame(img, ref) and _same_frame(other, ref), k
        assert not cull_raw.scene_pack_active()
        assert bool(r._frame.flags & 256) == bool(cull_raw._frame.flags & 256) == (k >= 1), k
        assert r.scene_pack_active() == (k >= 1), k
        assert not st.cull_fallback and not st_raw.cull_fallback and st.overflow == 0, (k, st)
        assert (st.pairs, st.visible) == (st_raw.pairs, st_raw.visible), (k, st, st_raw)
        if k >= 1:
            assert st.pairs < 0.6 * off.stats().pairs, (k, st)


# ------------------------------------------------------------------------------------------ several rounds, several chunks
@pytest.mark.parametrize("qcap", [None, 512])
def test_culled_rounds_chunks_and_the_gated_second_pass(gpu, monkeypatch, qcap):
    """800,000 Gaussians at 640 x 384: slices of 3,328 (phase A's loop goes round again; the last slice is partial), and with
    GS_OCC_QCAP = 512 seven chunks per slice.  Static pose, a creeping pose (dilated cuts) and a jump with the policy lifted,
    whose frame falls back: that is the PACKED gated second pass (frame_project_count_kernel<false, true> behind the gate).
    Every image equals the renderer with the cull off and the pack off.

    Observed on an MI355X, both parametrisations alike: 8 of the 9 frames culled, 5 dilated, 1 fell back (the jump to 25
    degrees), 4 dilated and clean."""
    if qcap is None:
        monkeypatch.delenv("GS_OCC_QCAP", raising=False)
    else:
        monkeypatch.setenv("GS_OCC_QCAP", str(qcap))
    n, w, h = 800_000, 640, 384
    params = _opaque(gpu, n, w, h, seed=5)
    kw = dict(max_pairs=4_500_000, auto_grow=False)
    r, off = FrameRenderer(gpu, **kw), FrameRenderer(gpu, scene_pack=False, occlusion_cull=False, **kw)
    r.CULL_MAX_SHIFT_PX = float("inf")
    yaws = [0.0, 0.0, 0.0, 0.01, 0.02, 0.03, 25.0, 25.0, 25.01]
    culled = fell = dilated = clean_dilated = 0
    for k, yaw in enumerate(yaws):
        cam = make_camera(w, h, yaw_deg=yaw)
        r._cull_off_until = 0
        img, _ = r.forward(*params, cam)
        st = r.stats()
        ref, _ = off.forward(*params, cam)
        assert off.stats().overflow == 0 and st.overflow == 0, (k, st)
        assert _same_frame(img, ref), (k, yaw, st)
        assert r.scene_pack_active() == (k >= 1), k
        is_culled, is_dilated = bool(r._frame.flags & 256), bool(r._frame.flags & 512)
        culled += int(is_culled)
        dilated += int(is_dilated)
        fell += int(st.cull_fallback)
        clean_dilated += int(is_dilated and not st.cull_fallback)
    print("scene pack, rounds and chunks:", qcap, "| culled", culled, "dilated", dilated, "fell back", fell,
          "dilated and clean", clean_dilated)
    assert culled == len(yaws) - 1, culled
    assert fell >= 1 and clean_dilated >= 4, (culled, dilated, fell, clean_dilated)


# ------------------------------------------------------------------------------------------ degenerate Gaussians
def test_degenerate_gaussians(gpu):
    """NaN and infinite positions and scales, zero quaternions, zero and huge scales, opa = +-inf on about 1 % of the scene: the
    pack holds whatever the exact arithmetic makes of them (a non-finite scale stores smax = NaN: projected, as the raw kernel's
    guard has it), and culled and unculled packed frames equal the raw renderer's bit for bit, NaN pixels included."""
    scene = _opaque_arrays()
    pos, quat, scale, opa = scene.pos.copy(), scene.quat.copy(), scene.scale.copy(), scene.opa.copy()
    k = 175
    idx = np.random.default_rng(9).choice(N, size=8 * k, replace=False).reshape(8, k)
    with np.errstate(all="ignore"):
        pos[idx[0]] = np.nan
        pos[idx[1], 2] = np.inf
        scale[idx[2]] = 0.0
        scale[idx[3]] = 1e30
        scale[idx[4], 1] = np.nan
        scale[idx[5], 0] = np.inf
        quat[idx[6, : k // 2]] = 0.0
        quat[idx[6, k // 2:], 2] = np.nan
        opa[idx[7, : k // 2]] = np.inf
        opa[idx[7, k // 2:]] = -np.inf
    params = [torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in (pos, quat, scale, opa, scene.rgb)]
    kw = dict(max_pairs=1 << 22, auto_grow=False)
    r_cull, r_flat = FrameRenderer(gpu, **kw), FrameRenderer(gpu, occlusion_cull=False, **kw)
    off = FrameRenderer(gpu, scene_pack=False, occlusion_cull=False, **kw)
    r_cull.CULL_MAX_SHIFT_PX = float("inf")
    culled = 0
    for j, yaw in enumerate((0.0, 0.0, 0.0, 0.02, 0.05, 3.0, 3.0)):
        cam = make_camera(W, H, yaw_deg=yaw)
        ref, _ = off.forward(*params, cam)
        assert off.stats().overflow == 0
        r_cull._cull_off_until = 0
        for r in (r_cull, r_flat):
            img, _ = r.forward(*params, cam)
            st = r.stats()
            assert st.overflow == 0 and r.scene_pack_active() == (j >= 1), (j, st)
            assert _same_frame(img, ref), (j, yaw, r is r_cull, st)
        culled += int(bool(r_cull._frame.flags & 256))
    assert culled == 6, culled


# ------------------------------------------------------------------------------------------ invalidation
def _arm(r, params, cam, frames=3):
    for _ in range(frames):
        r.forward(*params, cam, training=False)
    assert r.scene_pack_active()


def _check_rearm(gpu, r, params, cam, what):
    """After the parameters changed: the next frame renders raw and equals a fresh raw renderer on the CURRENT values, the one
    after it has a new pack and equals it too."""
    ref = _fresh_raw(gpu, params, cam)
    for k in range(3):
        img, _ = r.forward(*params, cam, training=False)
        assert r.scene_pack_active() == (k >= 1), (what, k)
        assert _same_frame(img, ref), (what, k)
    return ref


def test_pack_is_dropped_when_the_parameters_change(gpu):
    cam = make_camera(W, H)
    flat = FlatGaussianParams(_opaque(gpu))  # the five rendered tensors are views of one flat buffer
    params = flat.params
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS)
    _arm(r, params, cam)
    first = r.forward(*params, cam, training=False)[0].clone()

    # 1. an in-place torch write
    with torch.no_grad():
        params[0].add_(0.01)
    ref = _check_rearm(gpu, r, params, cam, "add_")
    assert not _same_frame(ref, first)  # (the change is one the image shows: a stale pack would have been caught)

    # 2. a native Adam step on the flat buffer (gs_adam_step_sharded through gs_train.FusedAdam)
    opt = FusedAdam(flat, base_lrs(TrainOptions()))
    flat.flat_grad.normal_(generator=torch.Generator(device=gpu).manual_seed(3))
    before = flat.flat_param.clone()
    opt.step()
    assert not torch.equal(before, flat.flat_param)
    ref2 = _check_rearm(gpu, r, params, cam, "FusedAdam.step")
    assert not _same_frame(ref2, ref)
    before = flat.flat_param.clone()
    opt.step_slice(0, advance=True)  # (gs_adam_step_multi)
    assert not torch.equal(before, flat.flat_param)
    ref2 = _check_rearm(gpu, r, params, cam, "FusedAdam.step_slice")

    # 3. the fused backward + Adam step of a training renderer on the same tensors
    tr = FrameRenderer(gpu, max_pairs=MAX_PAIRS, training=True, auto_grow=True)
    tr.forward(*params, cam)
    gimg = torch.randn(H, W, 3, device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    before = flat.flat_param.clone()
    tr.backward_adam(gimg, opt.fused_descriptor())
    assert not torch.equal(before, flat.flat_param) and not tr.scene_pack_active()
    ref3 = _check_rearm(gpu, r, params, cam, "backward_adam")
    assert not _same_frame(ref3, ref2)

    # 6. a training frame on the SAME renderer reads no pack and equals a raw training frame, image_padded included; the
    # inference frame behind it re-uses the pack
    img_t, pad_t = r.forward(*params, cam, training=True)
    assert not r.scene_pack_active()
    raw_t = FrameRenderer(gpu, max_pairs=MAX_PAIRS, scene_pack=False, training=True)
    img_r, pad_r = raw_t.forward(*params, cam)
    assert _same_frame(img_t, img_r) and _same_frame(pad_t, pad_r)
    img, _ = r.forward(*params, cam, training=False)
    assert r.scene_pack_active() and _same_frame(img, ref3)

    # 4. the five tensors deleted, new ones of the same shapes with other values (their addresses may or may not come back)
    shapes = [tuple(t.shape) for t in params]
    del flat, params, opt, tr, raw_t
    other = _opaque(gpu, seed=22)
    assert [tuple(t.shape) for t in other] == shapes
    ref4 = _check_rearm(gpu, r, other, cam, "new tensors")
    assert not _same_frame(ref4, ref3)

    # 5. another N
    fewer = [t[: N - 1000].contiguous() for t in other]
    _check_rearm(gpu, r, fewer, cam, "another N")


# ------------------------------------------------------------------------------------------ streams and capture
def test_pack_built_on_one_stream_is_read_on_another(gpu):
    params = _opaque(gpu)
    cam = make_camera(W, H)
    ref = _fresh_raw(gpu, params, cam)
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    with torch.cuda.stream(s1):
        r.forward(*params, cam)
        img1, _ = r.forward(*params, cam)  # builds on s1
        assert r.scene_pack_active()
    s2.wait_stream(s1)  # (the workspace is the renderer's: frames of one renderer are ordered by the caller)
    with torch.cuda.stream(s2):
        img2, _ = r.forward(*params, cam)
        assert r.scene_pack_active()
        img3, _ = r.forward(*params, cam)
    torch.cuda.synchronize()
    assert _same_frame(img1, ref) and _same_frame(img2, ref) and _same_frame(img3, ref)


def test_no_pack_is_built_inside_a_capture(gpu):
    """A frame captured into a graph never enqueues a build: the second consecutive frame of a key, captured, renders raw.
    (State only: the graph is not replayed.)"""
    params = _opaque(gpu)
    cam = make_camera(W, H)
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False, occlusion_cull=False)
    r.forward(*params, cam)
    assert not r.scene_pack_active()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.forward(*params, cam)
        assert not r.scene_pack_active() and r._pack is None
        r.forward(*params, cam)
        assert not r.scene_pack_active() and r._pack is None
    torch.cuda.synchronize()
    ref = _fresh_raw(gpu, params, cam)
    for k in range(2):  # outside the capture the next frame of the key (not its first) builds the pack
        img, _ = r.forward(*params, cam)
        assert r.scene_pack_active() and _same_frame(img, ref), k
