"""A frame does not depend on the renderer's earlier frames: frame k of every history of tests/frame_history.py, rendered by
ONE FrameRenderer that has been through frames 0 .. k-1 -- other sizes, Gaussian counts, colour dimensions, modes, poses,
capacities --, equals BIT FOR BIT frame k rendered alone by a renderer that has seen nothing else (image, padded image,
depth / alpha maps, every gradient, the pose gradient; the visible count, and the pair count of frames that were not occlusion
culled).  The fresh renderer's image of every distinct (scene, camera) is compared with the oracle once, within
test_gpu_frame.IMG_ATOL -- the only tolerance here --, so that the two renderers cannot be wrong together.  The same
histories run through gs_frame_forward on one 0xFF-filled workspace separate a leak in the library from a leak in a Python
cache.  tests/test_frame_history_host.py proves the catalogue valid on the CPU.

Every history asserts that it crossed the regimes it is about.  One ``HISTORY`` line per frame: index, scene, camera, mode,
flags, max_pairs, binning variant (profiles/frame_history.txt)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frame_history as FH
from gaussian import _lib
from gs_frame import FrameRenderer
from test_frame_history_host import CULL_MAX_SHIFT_PX, CULL_MIN_GAIN, CULL_NEAR_SHIFT_PX, LONG_LIST_FLAG_AT, LONG_SORT_FLAG_AT
from test_gpu_frame import IMG_ATOL

pytestmark = pytest.mark.gpu

CULL, DILATE, NEAR, PACK, REPEAT = (_lib.GS_FRAME_OCCLUSION_CULL, _lib.GS_FRAME_CULL_DILATE, _lib.GS_FRAME_CULL_DILATE_NEAR,
                                    _lib.GS_FRAME_SCENE_PACK, _lib.GS_FRAME_CULL_REPEAT)
ROWS, LONG_SORT, LONG_LISTS, PP = (_lib.GS_FRAME_BWD_ROWS, _lib.GS_FRAME_LONG_SORT, _lib.GS_FRAME_LONG_LISTS,
                                   _lib.GS_FRAME_PRINCIPAL_POINT)
GRAD_NAMES = ("grad_pos", "grad_quat", "grad_scale", "grad_opa", "grad_rgb")


def test_the_restated_thresholds_are_the_renderers():
    assert (FrameRenderer.LONG_SORT_FLAG_AT, FrameRenderer.LONG_LIST_FLAG_AT) == (LONG_SORT_FLAG_AT, LONG_LIST_FLAG_AT)
    assert (FrameRenderer.CULL_NEAR_SHIFT_PX, FrameRenderer.CULL_MAX_SHIFT_PX) == (CULL_NEAR_SHIFT_PX, CULL_MAX_SHIFT_PX)
    assert FrameRenderer.CULL_MIN_GAIN == CULL_MIN_GAIN


@functools.lru_cache(maxsize=None)
def _loss_grads(gpu, width, height):
    """(dL/dimage, dL/ddepth, dL/dalpha) for frames of this size: made once, shared, never written."""
    g = torch.Generator(device=gpu).manual_seed(1000 * width + height)
    return tuple(torch.randn(*shape, device=gpu, generator=g) / (width * height)
                 for shape in ((height, width, 3), (height, width), (height, width)))


def _frame(r, params, cam, mode, gpu):
    """Render one frame of ``mode`` with ``r`` -> {name: tensor} of everything the frame produced."""
    training, aux = mode in FH.TRAINING, mode in FH.AUX
    res = r.forward(*params, cam, training=training, aux=aux)
    out = {"image": res[0]}
    if training:
        out["padded"] = res[1]
    if aux:
        out["depth"], out["alpha"] = res[2], res[3]
        if training:
            out["aux_padded"] = r._aux_keep[2]
    if mode in ("Tb", "Tab", "Tp"):
        gimg, gd, ga = _loss_grads(gpu, int(cam.width), int(cam.height))
        kw = {}
        if mode == "Tab":
            kw = dict(grad_depth=gd, grad_alpha=ga)
        if mode == "Tp":
            out["grad_rot"], out["grad_tran"] = torch.empty(3, 3, device=gpu), torch.empty(3, device=gpu)
            kw = dict(grad_pose=(out["grad_rot"], out["grad_tran"]))
        out.update(zip(GRAD_NAMES, r.backward(gimg, **kw)))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(gpu, h, force_strips, auto_grow, bwd_rows=None):
    """Render the history ``h`` with one renderer R and every frame again with a fresh one; assert the property; -> (R, one
    record per frame: flags, max_pairs, variant, stats)."""
    tensors = FH.history_tensors(h, gpu)
    cams = FH.HistoryCameras()
    ctor = dict(max_pairs=h.max_pairs, auto_grow=auto_grow, force_strips=force_strips, bwd_rows=bwd_rows)
    R = FrameRenderer(gpu, **ctor)
    records, differs = [], []
    for k, s in enumerate(h.steps):
        what = (h.name, k, s.scene, s.camera, s.mode)
        params, cam = tensors[s.scene], cams.get(s.camera)
        got = _frame(R, params, cam, s.mode, gpu)
        st = R.stats()
        flags, cap, variant = int(R._frame.flags), int(R._frame.max_pairs), R.binning_variant()
        print(f"HISTORY {h.name} strips={int(bool(force_strips))} grow={auto_grow} rows={bwd_rows} | {k:2d} {s.scene:5s} "
              f"{s.camera:9s} {s.mode:3s} flags={flags:#07x} max_pairs={cap} {variant}")
        assert not R._long_lists_seen and not (flags & LONG_LISTS), what
        # frame k alone: R's constructor arguments, R's capacity at this moment, the backward kernel R's frame took (the latch
        # may move at stats() calls and the two kernels sum in different orders: the result GIVEN the kernel is what is pinned)
        fresh_kw = dict(ctor, max_pairs=cap, bwd_rows=bool(flags & ROWS))
        if k in h.overflow and not h.grows:
            fresh_kw["auto_grow"] = False  # (a fresh "async" renderer checks its FIRST frame and would grow: R did not)
        F = FrameRenderer(gpu, **fresh_kw)
        want = _frame(F, params, FH.camera(s.camera), s.mode, gpu)
        fst = F.stats()
        assert int(F._frame.max_pairs) == cap and not (int(F._frame.flags) & (CULL | PACK | LONG_SORT | LONG_LISTS)), what
        assert sorted(got) == sorted(want), what
        # (every frame of the history is rendered before the verdict: the failure names all the frames that differ)
        differs += [(k, s.scene, s.camera, s.mode, hex(flags), name) for name in got if not _same_bits(got[name], want[name])]
        if (st.visible, st.overflow) != (fst.visible, fst.overflow) or (not (flags & CULL) and st.pairs != fst.pairs):
            differs.append((k, s.scene, s.camera, s.mode, hex(flags), st, fst))
        assert not st.cull_unrepaired and R.broken_promises == 0, what
        if k in h.overflow and not h.grows:  # an overflowed frame is rendered EMPTY, not truncated
            assert st.overflow > cap and not any(bool(got[n].any()) for n in ("image", "padded") if n in got), what + (st,)
        records.append(dict(step=s, flags=flags, max_pairs=cap, variant=variant, stats=st))
        del F
    assert not differs, (h.name, "frames that differ from the frame rendered alone", differs)
    return R, records


def _assert_regimes(h, R, rec, force_strips, auto_grow):
    """The history crossed what it is about (``h.about``)."""
    flags = [r["flags"] for r in rec]
    names = [(r["step"].scene, FH.pose_name(r["step"].camera)) for r in rec]
    # The scene pack, and with it the repeat licence, belong to the strip variant (gs_frame_reads_scene_pack); in the table
    # variant -- the library's choice for these small scenes under force_strips=False -- the cull flag trims nothing, so the
    # renderer's own policy finds that the cull does not pay and backs off after the third frame at rest.
    if "cull" in h.about and force_strips:
        for bit, name in ((CULL, "OCCLUSION_CULL"), (DILATE, "CULL_DILATE"), (NEAR, "CULL_DILATE_NEAR"), (PACK, "SCENE_PACK")):
            assert any(f & bit for f in flags), (h.name, name, [hex(f) for f in flags])
        near, mid = names.index(("A", "C1near")), names.index(("A", "C1mid"))
        assert flags[near] & (CULL | DILATE | NEAR) == (CULL | DILATE | NEAR), hex(flags[near])
        assert flags[mid] & (CULL | DILATE | NEAR) == (CULL | DILATE), hex(flags[mid])
    if h.about & {"cull", "repeat"} and not force_strips:
        assert any(f & CULL for f in flags) and not any(f & (PACK | REPEAT) for f in flags), [hex(f) for f in flags]
        assert all(r["variant"] == "table" for r in rec)
    if "viewer" in h.about:
        # the ONE camera object moved in place: the renderer saw the new pose (by value) and flagged the frame by its shift --
        # in either variant: the policy's verdict on the frames at rest lands behind the description of the C1mid frame
        near, mid, far = (names.index(("A", c)) for c in ("C1near", "C1mid", "C1far"))
        assert flags[near - 1] & CULL and not (flags[near - 1] & DILATE), hex(flags[near - 1])
        assert flags[near] & (CULL | DILATE | NEAR) == (CULL | DILATE | NEAR), hex(flags[near])
        assert flags[mid] & (CULL | DILATE | NEAR) == (CULL | DILATE), hex(flags[mid])
        assert not (flags[far] & CULL) and not (flags[far + 1] & CULL), (hex(flags[far]), hex(flags[far + 1]))
        assert rec[far + 1]["step"].scene == "SH2"  # (... nor does the other scene's frame at that pose)
    if "far" in h.about:
        far = names.index(("A", "C1far"))
        assert not (flags[far] & CULL) and not (flags[far + 1] & CULL), (hex(flags[far]), hex(flags[far + 1]))
    if "reshape" in h.about:
        k = names.index(("A", "C2"))
        assert flags[k - 1] & CULL and not (flags[k] & CULL) and not (flags[k + 1] & CULL), [hex(f) for f in flags]
    if "repeat" in h.about and force_strips:
        assert R.cull_repeat_frames >= 1 and any(f & REPEAT for f in flags), (R.cull_repeat_frames, [hex(f) for f in flags])
        assert all((f & (CULL | PACK)) == (CULL | PACK) for f in flags if f & REPEAT)
    if "pile" in h.about:
        assert names[0] == ("PILE", "C1") and rec[0]["stats"].longest_list > LONG_SORT_FLAG_AT and R._long_sort_seen
        assert not (flags[0] & LONG_SORT) and all(f & LONG_SORT for f in flags[1:]), [hex(f) for f in flags]
    if "big" in h.about:
        # BIG runs the strip variant whatever the setting.  Under force_strips=False the frames in front of it run the table
        # variant; the frames behind it carry GS_FRAME_LONG_SORT -- 140,000 Gaussians on 48 tiles are lists of 2,842, beyond
        # LONG_SORT_FLAG_AT, and that latch is the renderer's for life -- and a frame with that flag takes the strip variant.
        first = [r["step"].scene for r in rec].index("BIG")
        assert first >= 1 and rec[first]["stats"].longest_list > LONG_SORT_FLAG_AT and R._long_sort_seen
        for k, r in enumerate(rec):
            assert bool(r["flags"] & LONG_SORT) == (k > first), (k, hex(r["flags"]))
            table = not force_strips and k < first
            assert r["variant"] == ("table" if table else "strip"), (k, r["step"], r["variant"])
    if "grow" in h.about:
        k = h.overflow[0]
        assert rec[k - 1]["max_pairs"] == h.max_pairs < rec[k]["stats"].pairs < rec[k]["max_pairs"], rec[k]
        assert rec[k]["stats"].overflow == 0 and R.overflowed_frames == 0  # redone in the larger workspace, not dropped
    if "overflow" in h.about:
        k = h.overflow[0]
        assert rec[k]["stats"].overflow > rec[k]["max_pairs"] == h.max_pairs, rec[k]
        assert all(r["stats"].overflow == 0 for j, r in enumerate(rec) if j != k)
        # auto_grow=False never looks; "async" finds the frame's counters in front of the next one and counts it
        assert R.overflowed_frames == (1 if auto_grow == "async" else 0)
        assert (rec[k + 1]["max_pairs"] > h.max_pairs) == (auto_grow == "async")


def _cases():
    for name, h in FH.HISTORIES.items():
        for strips in (True, False):
            for grow in h.auto_grow:
                yield pytest.param(name, strips, grow, id=f"{name}-{'strip' if strips else 'auto'}-grow_{grow}")


@pytest.mark.parametrize("name,force_strips,auto_grow", list(_cases()))
def test_frame_k_of_a_history_is_frame_k_rendered_alone(gpu, name, force_strips, auto_grow):
    h = FH.HISTORIES[name]
    R, rec = _run(gpu, h, force_strips, auto_grow)
    _assert_regimes(h, R, rec, force_strips, auto_grow)


@pytest.mark.parametrize("bwd_rows", [True, False])
@pytest.mark.parametrize("name", sorted(FH.HISTORIES))
def test_histories_with_the_backward_kernel_given(gpu, name, bwd_rows):
    """Every history once with bwd_rows=True and once with False (strip variant, the history's first auto_grow setting): the
    setting is part of the descriptor cache's key also where no backward reads it."""
    h = FH.HISTORIES[name]
    R, rec = _run(gpu, h, True, h.auto_grow[0], bwd_rows=bwd_rows)
    for r in rec:  # (the flag is every frame's; the library reads it on rgb training frames)
        assert bool(r["flags"] & ROWS) == bwd_rows, r


@pytest.mark.parametrize("force_strips", [True, False], ids=["strip", "auto"])
@pytest.mark.parametrize("name", [n for n, h in FH.HISTORIES.items() if False in h.auto_grow])
def test_a_history_issued_without_a_host_synchronisation(gpu, name, force_strips):
    """The whole history is issued by one renderer (auto_grow=False: nothing reads a counter) with no stats() call and no
    other renderer's frame in between, so that every frame starts while the library's side-stream work of the training forward
    before it -- the zero-fill of the gradient rows, the bucket list of a backward that may never come -- can still be in
    flight.  Only then is every frame rendered alone and compared, bit for bit.  (Which frames were culled depends here on when
    the policy's asynchronous counters land: the result must not.)"""
    h = FH.HISTORIES[name]
    tensors, cams = FH.history_tensors(h, gpu), FH.HistoryCameras()
    ctor = dict(max_pairs=h.max_pairs, auto_grow=False, force_strips=force_strips)
    R = FrameRenderer(gpu, **ctor)
    issued = []
    for s in h.steps:
        got = _frame(R, tensors[s.scene], cams.get(s.camera), s.mode, gpu)
        issued.append((s, got, int(R._frame.flags)))
    torch.cuda.synchronize()
    assert R.broken_promises == 0 and not R._long_lists_seen
    differs = []
    for k, (s, got, flags) in enumerate(issued):
        F = FrameRenderer(gpu, **dict(ctor, bwd_rows=bool(flags & ROWS)))
        want = _frame(F, tensors[s.scene], FH.camera(s.camera), s.mode, gpu)
        assert sorted(got) == sorted(want), (name, k, s)
        differs += [(k, s.scene, s.camera, s.mode, hex(flags), n) for n in got if not _same_bits(got[n], want[n])]
    assert not differs, (name, "frames that differ from the frame rendered alone", differs)


# ------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("scene,camera", [fc for fc in FH.distinct_frames() if fc[0] != "BIG"], ids=lambda v: v)
def test_the_fresh_renderers_image_is_the_oracles(gpu, scene, camera):
    """Once per distinct (scene, camera), so that the history renderer and the fresh one cannot be wrong together.  (BIG is
    compared with the fresh renderer only.)"""
    from gs_testutil import to_torch

    of = FH.oracle_frame(scene, camera)
    F = FrameRenderer(gpu, max_pairs=1 << 18, auto_grow=False)
    image, _ = F.forward(*to_torch(FH.scene(scene), gpu), FH.camera(camera))
    st = F.stats()
    err = float(np.abs(image.cpu().numpy() - of.image).max())
    print(f"frame history oracle {scene} {camera}: max |image - oracle| {err:.3g}")
    assert (st.visible, st.pairs, st.overflow) == (int(of.mask.sum()), len(of.ids), 0)
    assert err < IMG_ATOL, err


# ------------------------------------------------------------------------------------------------------------ at the C ABI
def _counters(f, tag, host):
    _lib.check(_lib.gs_frame_stats_tagged_async(C.byref(f), tag, host.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "gs_frame_stats_tagged_async")
    torch.cuda.synchronize()
    h = host.tolist()
    assert int(h[11]) & 0xffffffff == tag
    return int(h[0]), int(h[1]), int(h[2])


def _abi_forward(f, buf, gpu, host, tag):
    """``f`` through gs_frame_forward on the workspace ``buf`` -> (image, padded or None, (visible, pairs, overflow))."""
    g = _lib.GsFrameDP()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(_lib.GsFrameDP))
    base = buf.data_ptr()
    g.workspace = (base + 255) // 256 * 256
    g.workspace_bytes = buf.numel() - (g.workspace - base)
    image = torch.empty(g.height, g.width, 3, device=gpu)
    padded = torch.empty((g.height + 15) // 16 * 16, (g.width + 15) // 16 * 16, 3, device=gpu) if g.training else None
    g.image, g.image_padded = image.data_ptr(), (padded.data_ptr() if padded is not None else None)
    _lib.check(_lib.gs_frame_forward(C.byref(g), torch.cuda.current_stream().cuda_stream), "gs_frame_forward")
    counters = _counters(g, tag, host)  # (synchronises the device: the library's side stream included)
    return image, padded, counters


@pytest.mark.parametrize("name", sorted(FH.HISTORIES))
def test_library_frames_on_one_workspace_do_not_depend_on_its_earlier_frames(gpu, name):
    """The history's inference and training forwards through gs_frame_forward with flags 0 (a principal point keeps its flag:
    it is part of the camera) on ONE workspace buffer, sized for the largest descriptor and filled with 0xFF once: descriptors
    of changing (N, W, H, color_dim, training) find the previous frame's bytes under other names.  Each equals the same
    descriptor on a freshly 0xFF-filled buffer.  A helper renderer only FILLS IN the descriptors (through its own caches); the
    same descriptor object then runs on both buffers, so no Python state stands between the two frames that are compared.
    Ia and Tab steps run here as plain inference / training forwards, without GS_FRAME_AUX."""
    h = FH.HISTORIES[name]
    tensors = FH.history_tensors(h, gpu)
    d = FrameRenderer(gpu, max_pairs=h.max_pairs, auto_grow=False, occlusion_cull=False, scene_pack=False, force_strips=False)
    frames = []
    for s in h.steps:
        training = s.mode in FH.TRAINING
        f = d._describe(*tensors[s.scene], FH.camera(s.camera), training)
        f.flags &= PP
        frames.append((s, f, _lib.gs_frame_workspace_bytes(int(f.N), int(f.max_pairs), int(f.width), int(f.height),
                                                            int(f.color_dim), int(training))))
    size = max(need for _, _, need in frames) + 256
    assert len({need for _, _, need in frames}) > 1 or len({s.shape() for s in h.steps}) == 1, "one layout only"
    shared = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)
    host = torch.zeros(_lib.GS_STATS_TAGGED_N, dtype=torch.int64).pin_memory()
    for k, (s, f, _) in enumerate(frames):
        got = _abi_forward(f, shared, gpu, host, 2 * k + 1)
        clean = torch.full((size,), 0xFF, dtype=torch.uint8, device=gpu)
        want = _abi_forward(f, clean, gpu, host, 2 * k + 2)
        what = (name, k, s)
        assert _same_bits(got[0], want[0]), what + ("image",)
        assert (got[1] is None) == (want[1] is None) and (got[1] is None or _same_bits(got[1], want[1])), what + ("padded",)
        assert got[2] == want[2], what + (got[2], want[2])
        assert (got[2][2] != 0) == (k in h.overflow), what + (got[2],)
        del clean
    torch.cuda.synchronize()
