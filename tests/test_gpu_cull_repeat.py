"""GPU tier of GS_FRAME_CULL_REPEAT (include/gs_abi.h): an occlusion-culled frame that repeats the previous forward of its
workspace is issued without the five gated launches of its second pass.

Library level (descriptors flagged by hand, taken from a renderer that never flags): a kept promise is the unculled frame
bit for bit with every counter and the cut table of the unflagged culled frame; a broken one is reported, not repaired, and
the next unflagged frame is exact; a refusal enqueues nothing.  FrameRenderer: a camera at rest is flagged within 64 frames
without a single synchronising stats() call; every event that voids the evidence drops the licence until new evidence
arrives; a flagged run that runs past is noticed by the health probe.

Scenes: test_gpu_frame._dense_case (60,000 opaque Gaussians at 192 x 128: the strip variant when culled) and the ragged
300 x 232 frame of test_gpu_scene_pack (140,000 Gaussians).  Every image comparison is bit for bit against a renderer with the
cull and the scene pack off."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_geometry import pose_ctypes
from gs_scene import make_camera
from gs_testutil import to_torch
from test_gpu_frame import _dense_case
from test_gpu_scene_pack import _opaque, _same_frame

pytestmark = pytest.mark.gpu

CULL, DILATE, REPEAT, AUX, PACK = (_lib.GS_FRAME_OCCLUSION_CULL, _lib.GS_FRAME_CULL_DILATE, _lib.GS_FRAME_CULL_REPEAT,
                                   _lib.GS_FRAME_AUX, _lib.GS_FRAME_SCENE_PACK)
MAX_PAIRS = 1 << 20
SIZES = {"dense": (192, 128), "ragged": (300, 232)}


@functools.lru_cache(maxsize=None)
def _dense_arrays():
    return _dense_case()[0]


def _params(gpu, size):
    """Fresh device tensors of the (cached, never modified) scene of `size`."""
    if size == "dense":
        return to_torch(_dense_arrays(), gpu)
    return _opaque(gpu, 140_000, *SIZES[size])


def _cam(size, yaw=0.0):
    return make_camera(*SIZES[size], yaw_deg=yaw)


def _reference(gpu, params, cam, aux=False):
    off = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False, occlusion_cull=False, scene_pack=False)
    out = off.forward(*params, cam, aux=aux)
    return (out[0], out[2], out[3]) if aux else (out[0],)


def _same(a, b):
    return len(a) == len(b) and all(_same_frame(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ library level: by hand
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _copy(f, flags_on=0, flags_off=0, cam=None):
    """A copy of the descriptor `f` with fresh outputs (returned with it), other flags and, with `cam`, another pose."""
    g = _lib.GsFrameDP()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(_lib.GsFrameDP))
    g.flags = (g.flags | flags_on) & ~flags_off
    if cam is not None:
        g.rot, g.tran = pose_ctypes(cam)  # (rgb scenes: no other field of the descriptor depends on the pose)
    dev = torch.device("cuda", torch.cuda.current_device())
    outs = [torch.full((g.height, g.width, 3), -7.0, device=dev)]
    g.image = outs[0].data_ptr()
    if g.flags & AUX:
        outs += [torch.full((g.height, g.width), -7.0, device=dev) for _ in range(2)]
        g.depth, g.alpha = outs[1].data_ptr(), outs[2].data_ptr()
    return g, tuple(outs)


_HOST = None


def _counters(f, tag):
    """(visible, pairs, overflow, ran_past) of the last forward on f's workspace (synchronises)."""
    global _HOST
    if _HOST is None:
        _HOST = torch.zeros(_lib.GS_STATS_TAGGED_N, dtype=torch.int64).pin_memory()
    _lib.check(_lib.gs_frame_stats_tagged_async(C.byref(f), tag, _HOST.data_ptr(), _stream()), "gs_frame_stats_tagged_async")
    torch.cuda.synchronize()
    h = _HOST.tolist()
    assert int(h[11]) & 0xffffffff == tag
    return int(h[0]), int(h[1]), int(h[2]), int(h[10])


def _second_pass(f):
    out = C.c_int32(-1)
    assert _lib.gs_frame_cull_second_pass(C.byref(f), C.byref(out)) == 0
    return out.value


def _culled_renderer(gpu, params, cam, aux=False, frames=3):
    """A renderer that never flags, after an unculled and `frames - 1` culled frames at `cam`: its last descriptor is the
    unflagged culled frame of this pose -- trimmed by a culled frame's own cuts, read from a pack."""
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False, cull_second_pass="always")
    ref = _reference(gpu, params, cam, aux)
    for k in range(frames):
        r._cull_off_until = 0  # (the adaptive policy kept out of the way: which frames are culled does not depend on timing)
        out = r.forward(*params, cam, aux=aux)
        got = (out[0], out[2], out[3]) if aux else (out[0],)
        st = r.stats()
        assert _same(got, ref) and not st.cull_fallback and not st.cull_unrepaired and st.overflow == 0, (k, st)
        assert bool(r._frame.flags & CULL) == (k >= 1) and r.scene_pack_active() == (k >= 1) and not (r._frame.flags & REPEAT)
    assert r.binning_variant() == "strip" and not (r._frame.flags & DILATE) and r.cull_repeat_frames == 0
    return r, ref, st


@pytest.mark.parametrize("size,aux", [("dense", False), ("ragged", False), ("dense", True)])
def test_a_kept_promise_is_the_unculled_frame(gpu, size, aux):
    """An unculled frame, culled frames, then three frames flagged by hand at the same pose, from the pack: each image (and,
    with GS_FRAME_AUX, depth and alpha map) is the frame of a renderer with the cull and the pack off, nothing ran past, and
    visible count, emitted pairs and the cut table are those of the unflagged culled frame."""
    params, cam = _params(gpu, size), _cam(size)
    r, ref, st = _culled_renderer(gpu, params, cam, aux)
    cuts = r.cut_table().clone()
    assert int((cuts != -1).sum()) > cuts.numel() // 2  # (tiles saturate: there is something to trim by)
    assert _second_pass(r._frame) == 1
    for k in range(3):
        f, outs = _copy(r._frame, REPEAT)
        assert _second_pass(f) == 0
        _lib.check(_lib.gs_frame_forward(C.byref(f), _stream()), "gs_frame_forward")
        visible, pairs, overflow, ran_past = _counters(f, 100 + k)
        assert ran_past == 0 and overflow == 0 and (visible, pairs) == (st.visible, st.pairs), (k, visible, pairs, st)
        assert _same(outs, ref), (size, aux, k)
        assert torch.equal(r.cut_table(), cuts), (size, aux, k)
    # ... and the renderer goes on from there: an unflagged culled frame, clean and exact
    r._cull_off_until = 0
    out = r.forward(*params, cam, aux=aux)
    st2 = r.stats()
    assert _same((out[0], out[2], out[3]) if aux else (out[0],), ref) and not st2.cull_fallback
    assert (st2.visible, st2.pairs) == (st.visible, st.pairs) and r._frame.flags & CULL


def test_a_broken_promise_is_reported_and_the_next_unflagged_frame_is_exact(gpu):
    """After culled frames at yaw 0, a frame at yaw 30 degrees with the tiles' own cuts (the jump used: 0 -> 30 degrees, the
    largest of the camera path of test_gpu_frame's "lifted" policy test), twice from the same cut table:
      unflagged: it runs past, falls back -- the second pass renders it again -- and is exact;
      flagged by hand: not a fault -- the defined wrong-image case.  The run-past counter is non-zero, nothing is repaired.
    The unflagged culled frames that follow the unrepaired one at yaw 30 are exact, and clean.

    Observed on an MI355X: the flagged frame reports ran_past = 1 and its image differs from the reference; the four
    unflagged frames behind it report ran_past 0, 0, 0, 0 and are exact.  That the FIRST of them is clean is not this scene's
    luck.  A tile of the unrepaired frame stopped at some Gaussian g of its trimmed list and left cut = 1.0625 d(g) (or no
    cut, if it ended live), so the next frame lists every Gaussian up to that depth -- the ones the unrepaired frame
    composited and the ones it missed in front of them --, and with more in front every pixel stops at g or earlier: it
    cannot run past, whatever the image of the frame before it was.  "Repaired as usual" therefore reads: exact, and a
    fallback only where the trimmed lists are too short, which the unflagged twin above shows on the same cut table."""
    params = _params(gpu, "dense")
    cam0, cam30 = _cam("dense"), _cam("dense", 30.0)
    r, _, st0 = _culled_renderer(gpu, params, cam0)
    ref30 = _reference(gpu, params, cam30)
    # the unflagged twin: trimmed by yaw 0's cuts, it falls back and is exact
    g, outs = _copy(r._frame, cam=cam30)
    assert _second_pass(g) == 1
    _lib.check(_lib.gs_frame_forward(C.byref(g), _stream()), "gs_frame_forward")
    _, _, overflow, ran_past = _counters(g, 190)
    assert ran_past != 0 and overflow == 0 and _same(outs, ref30), ran_past
    # yaw 0's cut table again (an unflagged culled frame of the renderer), then the flagged frame
    r._cull_off_until = 0
    r.forward(*params, cam0)
    assert r._frame.flags & CULL and not r.stats().overflow
    f, outs = _copy(r._frame, REPEAT, cam=cam30)
    assert _second_pass(f) == 0
    _lib.check(_lib.gs_frame_forward(C.byref(f), _stream()), "gs_frame_forward")
    host = torch.zeros(1, dtype=torch.int64).pin_memory()
    _lib.check(_lib.gs_frame_cull_fallback_async(C.byref(f), host.data_ptr(), _stream()), "gs_frame_cull_fallback_async")
    torch.cuda.synchronize()
    ran = int(host[0])
    print("flagged frame at yaw 30 after yaw 0: ran_past", ran, "| image equals the reference:", _same(outs, ref30))
    assert ran != 0, "the 30-degree jump did not run past on this scene"
    # the same descriptor without the flag: the second pass is enqueued again
    fell = []
    for k in range(4):
        g, outs = _copy(f, 0, REPEAT)
        assert _second_pass(g) == 1
        _lib.check(_lib.gs_frame_forward(C.byref(g), _stream()), "gs_frame_forward")
        _, pairs, overflow, ran_past = _counters(g, 200 + k)
        fell.append(ran_past)
        assert overflow == 0 and _same(outs, ref30), (k, ran_past)
    print("unflagged culled frames at yaw 30 behind it: ran_past", fell)
    assert fell == [0, 0, 0, 0], fell  # (exact above; clean by the argument of the docstring)


def test_refusals_enqueue_nothing(gpu):
    """GS_FRAME_CULL_REPEAT with GS_FRAME_CULL_DILATE: GS_E_INVALID with the reason, the outputs and the workspace's counters
    untouched; the valid frame rendered afterwards equals the reference."""
    params, cam = _params(gpu, "dense"), _cam("dense")
    r, ref, st = _culled_renderer(gpu, params, cam)
    before = _counters(r._frame, 300)
    cuts = r.cut_table().clone()
    for extra in (DILATE, DILATE | _lib.GS_FRAME_CULL_DILATE_NEAR):
        f, outs = _copy(r._frame, REPEAT | extra)
        out = C.c_int32(-7)
        assert _lib.gs_frame_cull_second_pass(C.byref(f), C.byref(out)) == -1 and out.value == -7
        assert _lib.gs_frame_forward(C.byref(f), _stream()) == -1
        why = _lib.gs_last_error().decode()
        assert "GS_FRAME_CULL_REPEAT" in why and "GS_FRAME_CULL_DILATE" in why, why
        ms = (C.c_float * 6)()
        assert _lib.gs_frame_forward_profile(C.byref(f), ms, _stream()) == -1
        torch.cuda.synchronize()
        assert all(bool((o == -7.0).all()) for o in outs)
    assert _counters(r._frame, 301) == before and torch.equal(r.cut_table(), cuts)
    f, outs = _copy(r._frame, REPEAT)
    _lib.check(_lib.gs_frame_forward(C.byref(f), _stream()), "gs_frame_forward")
    assert _counters(f, 302) == before and _same(outs, ref)
    # the profiled forward honours the flag: six stage times, the same frame
    f, outs = _copy(r._frame, REPEAT)
    ms = (C.c_float * 6)()
    _lib.check(_lib.gs_frame_forward_profile(C.byref(f), ms, _stream()), "gs_frame_forward_profile")
    torch.cuda.synchronize()
    assert _same(outs, ref) and 0.0 < ms[4] < ms[5]


# ------------------------------------------------------------------------------------------ FrameRenderer
def _flagged(r):
    return bool(r._frame.flags & REPEAT)


def _run_until_flagged(r, params, cam, ref, limit=64, sync_every=4):
    """Frames at rest, no stats(): -> how many were issued before the first flagged one (asserted below `limit`).  Every image
    is compared with `ref` at the synchronisation points."""
    pending = []
    for k in range(limit):
        img, _ = r.forward(*params, cam)
        pending.append(img)
        flagged = _flagged(r)
        if flagged or k % sync_every == sync_every - 1:
            torch.cuda.synchronize()  # (so that the probes land: the host of a test runs far ahead of a 60-k scene's frames)
            assert all(_same_frame(i, ref[0]) for i in pending), k
            pending = []
        if flagged:
            return k
    raise AssertionError(f"no frame was flagged within {limit} frames: licence {r._repeat_licence is not None}, "
                         f"settled {r._cull_settled}, probe {r._cull_probe is not None}")


@pytest.mark.parametrize("size", ["dense", "ragged"])
def test_a_camera_at_rest_is_flagged_within_64_frames(gpu, size):
    params, cam = _params(gpu, size), _cam(size)
    ref = _reference(gpu, params, cam)
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False)
    first = _run_until_flagged(r, params, cam, ref)
    print(size, ": first flagged frame", first)
    assert 2 <= first < 64 and r.cull_repeat_frames == 1 and r._cull_settled
    culled, sp = C.c_int32(), C.c_int32()
    _lib.call("gs_frame_is_occlusion_culled", C.byref(r._frame), C.byref(culled))
    _lib.call("gs_frame_cull_second_pass", C.byref(r._frame), C.byref(sp))
    assert (culled.value, sp.value) == (1, 0) and r.scene_pack_active()
    imgs = []
    for k in range(2 * FrameRenderer.CULL_HEALTH_EVERY + 8):  # (across two health probes)
        imgs.append(r.forward(*params, cam)[0])
        assert _flagged(r), k
        if k % 8 == 7:
            torch.cuda.synchronize()
            assert all(_same_frame(i, ref[0]) for i in imgs), k
            imgs = []
    assert r.cull_repeat_frames == 1 + 2 * FrameRenderer.CULL_HEALTH_EVERY + 8 and r.broken_promises == 0
    st = r.stats()
    assert not st.cull_fallback and not st.cull_unrepaired and st.overflow == 0 and _flagged(r)
    # the profiled forward is a forward like any other: flagged, exact, the licence kept
    r.profile_forward(*params, cam)
    assert _flagged(r) and _same_frame(r._keep[5], ref[0])
    r.forward(*params, cam)
    assert _flagged(r)
    # cull_second_pass="always": never
    a = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False, cull_second_pass="always")
    for k in range(16):
        img, _ = a.forward(*params, cam)
        assert not _flagged(a) and (k == 0 or a._frame.flags & CULL)
        if k % 4 == 3:
            torch.cuda.synchronize()
            assert _same_frame(img, ref[0])
    assert a.cull_repeat_frames == 0 and a._repeat_licence is None and a._cull_settled
    with pytest.raises(ValueError):
        FrameRenderer(gpu, cull_second_pass="never")


def _after_the_event(gpu, r, params, cam, what):
    """The licence is gone; the next frames are unflagged and exact on the CURRENT parameters; it returns with new evidence."""
    assert r._repeat_licence is None, what
    ref = _reference(gpu, params, cam)
    for k in range(2):  # (the earliest evidence: the second frame of the new key is probed, its counters land behind it)
        img, _ = r.forward(*params, cam)
        torch.cuda.synchronize()
        assert not _flagged(r) and _same_frame(img, ref[0]), (what, k)
    first = _run_until_flagged(r, params, cam, ref)
    print(what, ": flagged again after", 2 + first, "frames")
    return ref


def test_every_event_that_voids_the_evidence_drops_the_licence(gpu):
    cam = _cam("dense")
    params = _params(gpu, "dense")
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False)
    ref = _reference(gpu, params, cam)
    _run_until_flagged(r, params, cam, ref)

    # 1. a torch in-place edit of a parameter tensor (bumps `_version`: the pack build is void)
    with torch.no_grad():
        params[0].add_(0.01)
    img, _ = r.forward(*params, cam)
    assert not _flagged(r) and not r.scene_pack_active()
    ref1 = _after_the_event(gpu, r, params, cam, "add_")
    assert _same_frame(img, ref1[0]) and not _same_frame(ref1[0], ref[0])

    # 2. a pose change of 0.002 degree and the return to the old pose
    near = _cam("dense", 0.002)
    ref_near = _reference(gpu, params, near)
    img, _ = r.forward(*params, near)
    assert not _flagged(r) and r._frame.flags & DILATE and _same_frame(img, ref_near[0])
    img, _ = r.forward(*params, cam)
    assert not _flagged(r) and _same_frame(img, ref1[0])
    _after_the_event(gpu, r, params, cam, "pose and back")

    # 3. another max_pairs
    r.max_pairs += 4096
    img, _ = r.forward(*params, cam)
    assert not _flagged(r) and _same_frame(img, ref1[0])
    _after_the_event(gpu, r, params, cam, "max_pairs")

    # 4. a training forward in between
    r.forward(*params, cam, training=True)
    assert not _flagged(r)
    img, _ = r.forward(*params, cam)
    assert not _flagged(r) and not (r._frame.flags & CULL) and _same_frame(img, ref1[0])
    _after_the_event(gpu, r, params, cam, "training forward")

    # 5. a frame captured into a graph is never flagged, and voids the evidence
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.forward(*params, cam)
        assert not _flagged(r)
        r.forward(*params, cam)
        assert not _flagged(r)
    torch.cuda.synchronize()
    _after_the_event(gpu, r, params, cam, "stream capture")

    # 6. new tensors of the same shapes after the old ones were freed (their addresses may come back; other values)
    shapes = [tuple(t.shape) for t in params]
    del params, img
    other = [t + 0.003 if k == 0 else t for k, t in enumerate(_params(gpu, "dense"))]
    assert [tuple(t.shape) for t in other] == shapes
    img, _ = r.forward(*other, cam)
    assert not _flagged(r)
    ref6 = _after_the_event(gpu, r, other, cam, "new tensors")
    assert _same_frame(img, ref6[0]) and not _same_frame(ref6[0], ref1[0])
    assert r.broken_promises == 0


def test_the_health_probe_notices_a_broken_promise(gpu, monkeypatch):
    """A bookkeeping error, simulated: `_camera_shift_px` answers 0.0 for a camera that jumped by 30 degrees, so the renderer
    takes the jumped frames for repeats and flags them.  With a health probe on every flagged frame it notices within a few
    frames, warns once, counts one broken promise, withdraws the licence and backs the cull off; every frame from the first
    unflagged one on is exact."""
    params = _params(gpu, "dense")
    cam0, cam30 = _cam("dense"), _cam("dense", 30.0)
    r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False)
    _run_until_flagged(r, params, cam0, _reference(gpu, params, cam0))
    monkeypatch.setattr(r, "CULL_HEALTH_EVERY", 1, raising=False)
    monkeypatch.setattr(r, "_camera_shift_px", lambda camera: 0.0)
    ref30 = _reference(gpu, params, cam30)
    flagged, exact = [], []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k in range(12):
            img, _ = r.forward(*params, cam30)
            torch.cuda.synchronize()
            flagged.append(_flagged(r))
            exact.append(_same_frame(img, ref30[0]))
    print("jumped frames flagged", flagged, "exact", exact)
    ours = [w for w in caught if "GS_FRAME_CULL_REPEAT" in str(w.message)]
    assert flagged[0] and not all(flagged[:4]), flagged          # taken for a repeat; noticed within a few frames
    first_unflagged = flagged.index(False)
    assert not any(flagged[first_unflagged:]) and all(exact[first_unflagged:]), (flagged, exact)
    assert len(ours) == 1 and "frame " in str(ours[0].message), [str(w.message) for w in caught]
    assert r.broken_promises == 1 and r._repeat_licence is None
    assert r._cull_off_until > r._frame_serial and not r._cull_settled  # the cull's own back-off
