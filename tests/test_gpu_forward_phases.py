"""GPU tier: the forward issued in ranges of project slices is the one-call frame, bit for bit.

The view-parallel trainer renders every frame but its first as gs_frame_forward_project(f, slice_begin, slice_end) range by
range behind the optimizer of the previous step, then gs_frame_forward_rest (gs_frame.hip; FrameRenderer.forward_begin /
forward_finish; gs_train.Trainer._project_ahead).  A launch of the project stage covers slices [slice0, slice0 + S) and finds
a workgroup's slice with the XCD dealing permutation taken over the RANGE's length S (cull_project.hip, project_count_body);
the tile-order workgroup, the side-stream join and the counters' memset belong to the range that starts at slice 0.

`same_frame` renders one descriptor twice on two workspaces -- (a) one gs_frame_forward, (b) a partition of [0, slices) as
ranges + rest -- and compares bits: image, padded image, counters (visible, pairs, overflow, longest list), rectangle records,
tile ranges, emitted sorted keys and ids, and the five gradients of gs_frame_backward for one random dL/dimage.  Run (b) reads
its parameters from buffers that start all-NaN; the true values of a range's Gaussians are copied in, in stream order, right
before that range is issued -- what the trainer's situation is, made strict: when a range is launched the parameters of every
range not yet issued are not final.  Run (b)'s workspace starts zero-filled (0xFF in the dirty-workspace case), so that a
slice nobody projected shows as culled Gaussians and never as an earlier test's identical records.

Shapes are the smallest that cross each path (79 slices of 256 against range lengths below, at and above the eight XCDs;
per_slice 512 with a one-Gaussian last slice; the 256-slice limit; one and two slices).  profiles/forward_phases.txt lists the
cases with their plans and outcomes."""
import copy
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import oracle
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import OracleFrame, activate, frame_scalars, to_torch
from pp_testutil import offset_camera

pytestmark = pytest.mark.gpu

GS_E_INVALID = -1
NAMES = ("pos", "quat", "scale", "opa", "rgb")
KW = dict(training=True, auto_grow=False, force_strips=True, emit_sorted_keys=True, occlusion_cull=False, scene_pack=False)
W, H = 160, 112
N_BASE = 20_000          # 79 slices of 256 (gs_frame_layout.h, gs_strip_plan_for), the last one holds 32 Gaussians
LENGTHS = (1, 7, 8, 9, 13, 41)  # range lengths below 8, equal to 8, above 8 and no multiple of 8: strip_slice_of_block(blk, S)


def _stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def partition(lengths):
    out, s = [], 0
    for n in lengths:
        out.append((s, s + n))
        s += n
    return out


def first_then_descending(ranges):
    return [ranges[0]] + sorted(ranges[1:], reverse=True)


class Frame:
    """One training frame description on a renderer (workspace, side-stream handle) of its own, driven through the C ABI."""

    def __init__(self, gpu, params, cam, max_pairs=1 << 20, fill=None, **kw):
        self.gpu = gpu
        self.r = FrameRenderer(gpu, max_pairs=max_pairs, **{**KW, **kw})
        self.f = None
        self.describe(params, cam)
        if fill is not None:
            self.r._ws.fill_(fill)

    def describe(self, params, cam, max_pairs=None):
        """(Re)describe: other parameter buffers, another camera or a smaller capacity in the SAME workspace."""
        r = self.r
        if max_pairs is not None:
            assert max_pairs <= r.max_pairs  # (the workspace allocated for the larger capacity holds the smaller frame)
            r.max_pairs = max_pairs
        self.params = list(params)
        ws = r._ws
        f = r._describe(*self.params, cam, bool(r.training))
        assert ws is None or r._ws is ws
        g = r._grid
        nan = float("nan")  # every pixel is the frame's own or the comparison sees it
        self.image = torch.full((g.height, g.width, 3), nan, device=self.gpu)
        self.padded = torch.full((g.padded_height, g.padded_width, 3), nan, device=self.gpu) if r.training else None
        f.image = self.image.data_ptr()
        f.image_padded = self.padded.data_ptr() if self.padded is not None else None
        self.f, self.grid = f, g
        return self

    def plan(self):
        n_sl, per = C.c_int32(), C.c_int64()
        _lib.check(_lib.gs_frame_project_slices(C.byref(self.f), C.byref(n_sl), C.byref(per)), "gs_frame_project_slices")
        return n_sl.value, per.value

    def one_call(self):
        _lib.check(_lib.gs_frame_forward(C.byref(self.f), _stream(self.gpu)), "gs_frame_forward")
        return self

    def project(self, s0, s1):
        return _lib.gs_frame_forward_project(C.byref(self.f), s0, s1, _stream(self.gpu))

    def in_ranges(self, ranges, source=None):
        """The project stage range by range in the given order, then the rest.  ``source``: the true parameters; the rows
        of a range's Gaussians are copied into this frame's (NaN) buffers right before the range is issued."""
        n_sl, per = self.plan()
        assert ranges[0][0] == 0 and partition([b - a for a, b in sorted(ranges)]) == sorted(ranges)
        assert sorted(ranges)[-1][1] == n_sl, (ranges, n_sl)
        n = int(self.f.N)
        for s0, s1 in ranges:
            if source is not None:
                g0, g1 = s0 * per, min(s1 * per, n)
                for dst, src in zip(self.params, source):
                    dst[g0:g1].copy_(src[g0:g1])
            _lib.check(self.project(s0, s1), "gs_frame_forward_project")
        _lib.check(_lib.gs_frame_forward_rest(C.byref(self.f), _stream(self.gpu)), "gs_frame_forward_rest")
        return self

    def _view(self, ptr, nbytes, dtype):
        off = ptr.value - self.r._ws.data_ptr()
        assert 0 <= off and off + nbytes <= self.r._ws.numel()
        return self.r._ws[off:off + nbytes].view(dtype)

    def snapshot(self):
        """Copies of everything the forward left: {name: tensor or tuple}.  Synchronises."""
        f = self.f
        st, longest = torch.zeros(4, dtype=torch.int64).pin_memory(), torch.zeros(1, dtype=torch.int64).pin_memory()
        _lib.check(_lib.gs_frame_stats_async(C.byref(f), st.data_ptr(), _stream(self.gpu)), "gs_frame_stats_async")
        _lib.check(_lib.gs_frame_longest_list_async(C.byref(f), longest.data_ptr(), _stream(self.gpu)),
                   "gs_frame_longest_list_async")
        torch.cuda.synchronize(self.gpu)
        v, m, o = (int(x) for x in st.tolist()[:3])
        out = {"image": self.image.clone(), "stats": (v, m, o, int(longest[0])), "flags": (int(f.flags),)}
        if self.padded is not None:
            out["padded"] = self.padded.clone()
        rects = C.c_void_p()
        _lib.check(_lib.gs_frame_debug_rects(C.byref(f), C.byref(rects)), "gs_frame_debug_rects")
        out["rects"] = self._view(rects, 16 * int(f.N), torch.int32).clone()
        if o == 0:
            p = [C.c_void_p() for _ in range(7)]
            _lib.check(_lib.gs_frame_debug_views(C.byref(f), *[C.byref(x) for x in p]), "gs_frame_debug_views")
            assert p[0].value, "GS_FRAME_EMIT_SORTED_KEYS: the sorted keys are materialised"
            out["sorted_keys"] = self._view(p[0], 8 * m, torch.int64).clone()
            out["sorted_ids"] = self._view(p[1], 4 * m, torch.int32).clone()
            out["tile_ranges"] = self._view(p[2], 8 * self.grid.n_tiles, torch.int32).clone()
        return out

    def snapshot_image(self):
        torch.cuda.synchronize(self.gpu)
        return self.image.clone()

    def backward(self, grad_image):
        grads = [torch.full_like(t, float("nan")) for t in self.params]  # every element is written or the comparison sees it
        _lib.check(_lib.gs_frame_backward(C.byref(self.f), grad_image.data_ptr(), *(g.data_ptr() for g in grads),
                                          _stream(self.gpu)), "gs_frame_backward")
        return dict(zip(("grad_" + n for n in NAMES), grads))


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], tuple):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            assert a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def grad_image(gpu, g, seed=4):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(g.height, g.width, 3, device=gpu, generator=gen) / (g.height * g.width)


# ----------------------------------------------------------------------------------------------------------- the cases
def _base_scene(n=N_BASE, w=W, h=H, seed=7, **kw):
    return make_scene(n, w, h, seed=seed, **kw)


def _base_camera(w=W, h=H):
    cam = make_camera(w, h, yaw_deg=2.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    return cam


def _ragged_scene(n, w, h, seed):
    s = _base_scene(n, w, h, seed=seed)
    s.pos[-1] = (0.0, 0.0, 2.0)  # the one Gaussian of the last slice: in front of the camera, on its axis
    s.opa[-1] = 2.0
    return s


def _exp_scene():
    s = _base_scene(seed=13)
    s.scale = np.log(np.abs(s.scale) + 1e-4).astype(np.float32)
    return s


def _pp_camera():
    cam = _base_camera()
    cam.focal_y = float(np.float32(0.85 * cam.focal_x))
    return offset_camera(cam, (7.3, -4.6))


def _hidden_scene():
    s = _base_scene(seed=17)
    s.pos[3 * 256:6 * 256, 2] = -5.0  # the Gaussians of slices 3, 4 and 5: behind the camera
    return s


# name -> (scene factory, camera factory, renderer keywords, max_pairs)
CASES = {
    "base": (_base_scene, _base_camera, {}, 1 << 20),
    "n65537": (lambda: _ragged_scene(65_537, 256, 256, 5), lambda: _base_camera(256, 256), {}, 1 << 21),
    "n65536": (lambda: _base_scene(65_536, 256, 256, seed=6), lambda: _base_camera(256, 256), {}, 1 << 21),
    "n255": (lambda: _base_scene(255, 64, 48, seed=3), lambda: _base_camera(64, 48), {}, 1 << 16),
    "n257": (lambda: _ragged_scene(257, 64, 48, 3), lambda: _base_camera(64, 48), {}, 1 << 16),
    "dist": (lambda: _base_scene(seed=29), _base_camera, dict(tile_culling_method="dist", tile_culling_dist_thresh=0.5), 1 << 20),
    "exp": (_exp_scene, _base_camera, dict(scale_activation="exp"), 1 << 20),
    "sh27": (lambda: _base_scene(seed=11, use_sh=True, sh_degree=2), _base_camera, {}, 1 << 20),
    "sh48": (lambda: _base_scene(seed=11, use_sh=True, sh_degree=3), _base_camera, {}, 1 << 20),
    "pp": (lambda: _base_scene(seed=19), _pp_camera, {}, 1 << 20),
    "hidden": (_hidden_scene, _base_camera, {}, 1 << 20),
}
# name -> (slices, per_slice) by gs_strip_plan_for: per = ceil(ceil(N / 256) / 256) * 256, slices = ceil(N / per)
PLANS = {"base": (79, 256), "n65537": (129, 512), "n65536": (256, 256), "n255": (1, 256), "n257": (2, 256), "dist": (79, 256),
         "exp": (79, 256), "sh27": (79, 256), "sh48": (79, 256), "pp": (79, 256), "hidden": (79, 256)}


@functools.lru_cache(maxsize=None)
def _case_arrays(name):
    scene_of, cam_of, kw, max_pairs = CASES[name]
    return scene_of(), cam_of(), kw, max_pairs


_REF = {}


def reference(gpu, name):
    """Run (a) of a case -- one gs_frame_forward + gs_frame_backward on a workspace of its own --, computed once and shared:
    (true parameters on the device, camera, renderer keywords, max_pairs, dL/dimage, forward snapshot + gradients)."""
    if name not in _REF:
        scene, cam, kw, max_pairs = _case_arrays(name)
        params = to_torch(scene, gpu)
        a = Frame(gpu, params, cam, max_pairs, **kw)
        assert a.plan() == PLANS[name], (name, a.plan())
        assert _lib.gs_frame_binning_variant(C.byref(a.f)) == 4  # "strip"
        g = grad_image(gpu, a.grid)
        snap = a.one_call().snapshot()
        snap.update(a.backward(g))
        torch.cuda.synchronize(gpu)
        v, m, o, _ = snap["stats"]
        assert o == 0 and v > 0 and m > 0, (name, snap["stats"])
        assert bool(torch.isfinite(snap["image"]).all()) and bool(torch.isfinite(snap["padded"]).all())
        assert all(bool(torch.isfinite(snap["grad_" + n]).all()) for n in NAMES)
        assert float(snap["grad_pos"].abs().max()) > 0
        if name in ("n257", "n65537"):  # the last slice's one Gaussian is visible and listed: its slice matters
            assert int(snap["rects"].view(-1, 4)[-1, 2]) != 0 and int(snap["rects"].view(-1, 4)[-1, 3]) > 0
        _REF[name] = (params, cam, kw, max_pairs, g, snap)
    return _REF[name]


def sliced_frame(gpu, name, fill=0):
    """Run (b)'s frame of a case: all-NaN parameter buffers, a workspace filled with ``fill``."""
    params, cam, kw, max_pairs, _, _ = reference(gpu, name)
    nan_params = [torch.full_like(t, float("nan")) for t in params]
    return Frame(gpu, nan_params, cam, max_pairs, fill=fill, **kw)


def same_frame(gpu, name, ranges, fill=0):
    """Run (b) of case ``name`` with the partition ``ranges`` in the order given, against run (a).  -> run (b)'s snapshot"""
    params, _, _, _, g, want = reference(gpu, name)
    b = sliced_frame(gpu, name, fill)
    got = b.in_ranges(ranges, source=params).snapshot()
    got.update(b.backward(g))
    torch.cuda.synchronize(gpu)
    assert_same(want, got, (name, ranges[:4], len(ranges)))
    print("PHASES", name, "slices %d per_slice %d" % PLANS[name], "ranges", len(ranges), "first", ranges[:3], "stats",
          got["stats"], "equal")
    return got


BASE_RANGES = partition(LENGTHS)
ORDERS = {
    "in_order": BASE_RANGES,
    "descending": first_then_descending(BASE_RANGES),
    "singles": partition([1] * 79),
    "one_range": [(0, 79)],
}


def test_partition_crosses_the_dealing_permutation():
    """Conditions on the INPUT: the range lengths sit on both sides of the eight XCDs the permutation deals over."""
    assert sum(LENGTHS) == PLANS["base"][0] and BASE_RANGES[-1] == (38, 79)
    assert any(n < 8 for n in LENGTHS) and 8 in LENGTHS and any(n > 8 and n % 8 for n in LENGTHS)
    assert ORDERS["descending"] == [(0, 1), (38, 79), (25, 38), (16, 25), (8, 16), (1, 8)]


@pytest.mark.parametrize("order", list(ORDERS))
def test_range_lengths_against_the_dealing_permutation(gpu, order):
    same_frame(gpu, "base", ORDERS[order])


@pytest.mark.parametrize("ranges", [[(0, 1), (1, 128), (128, 129)], [(0, 1), (128, 129), (1, 128)]], ids=["in_order", "reversed"])
def test_per_slice_512_with_a_ragged_end(gpu, ranges):
    """65,537 Gaussians: 129 slices of 512, the last holds ONE Gaussian (and is a range of its own)."""
    same_frame(gpu, "n65537", ranges)


@pytest.mark.parametrize("ranges", [[(0, 128), (128, 256)], [(0, 255), (255, 256)]], ids=["halves", "255+1"])
def test_the_slice_limit(gpu, ranges):
    """65,536 Gaussians: GS_BIN_SLICES = 256 slices of 256, the most a frame is cut into."""
    same_frame(gpu, "n65536", ranges)


@pytest.mark.parametrize("name,ranges", [("n255", [(0, 1)]), ("n257", [(0, 1), (1, 2)])], ids=["255", "257"])
def test_tiny(gpu, name, ranges):
    same_frame(gpu, name, ranges)


@pytest.mark.parametrize("order", ["in_order", "descending"])
@pytest.mark.parametrize("name", ["dist", "exp", "sh27", "sh48", "pp"])
def test_instantiations(gpu, name, order):
    """The DIST instantiation of the project + count kernel, the exp activation, both SH widths, and a camera with fx != fy and
    an off-centre principal point (the _pp kernels)."""
    params, cam, _, _, _, _ = reference(gpu, name)
    b = same_frame(gpu, name, ORDERS[order])
    assert bool(b["flags"][0] & _lib.GS_FRAME_PRINCIPAL_POINT) == (name == "pp")
    if name == "pp":
        assert cam.focal_x != cam.focal_y
    if name.startswith("sh"):
        assert params[4].shape[1] == int(name[2:])
    assert b["stats"][1] > 0


def test_a_range_with_nothing_visible(gpu):
    scene, cam, _, _ = _case_arrays("hidden")
    qn, sn = activate(scene)
    _, hw, hh, _ = frame_scalars(cam)
    _, _, mask = oracle.global_culling(scene.pos, qn, sn, cam.rot, cam.tran, cam.near, hw, hh)
    mask = np.asarray(mask).astype(bool)
    assert not mask[3 * 256:6 * 256].any() and mask[:3 * 256].any() and mask[6 * 256:].any()
    got = same_frame(gpu, "hidden", [(0, 3), (6, 79), (3, 6)])
    assert got["stats"][0] == int(mask.sum())
    assert not bool((got["rects"].view(-1, 4)[3 * 256:6 * 256] != 0).any())  # all-zero rectangles: culled


def test_overflowing_frame_and_the_frame_after_it(gpu):
    """max_pairs below the frame's need: both runs report the same overflow and the same empty image; the next frame of the
    same workspaces, with room, is the base frame again -- (b) in ranges behind a training forward whose backward never came."""
    params, cam, kw, max_pairs, g, want = reference(gpu, "base")
    need = want["stats"][1]
    small = need // 3
    a = Frame(gpu, params, cam, max_pairs, **kw)
    nan_params = [torch.full_like(t, float("nan")) for t in params]
    b = Frame(gpu, nan_params, cam, max_pairs, fill=0, **kw)
    sa = a.describe(params, cam, small).one_call().snapshot()
    sb = b.describe(nan_params, cam, small).in_ranges(ORDERS["descending"], source=params).snapshot()
    assert sa["stats"][1] == 0 and sa["stats"][2] >= need > small, sa["stats"]
    assert float(sa["image"].abs().max()) == 0.0
    assert_same(sa, sb, "overflow")
    print("PHASES overflow max_pairs", small, "stats", sb["stats"], "equal")
    for t in nan_params:
        t.fill_(float("nan"))
    a.r.max_pairs = b.r.max_pairs = max_pairs
    sa = a.describe(params, cam).one_call().snapshot()
    sa.update(a.backward(g))
    sb = b.describe(nan_params, cam).in_ranges(ORDERS["descending"], source=params).snapshot()
    sb.update(b.backward(g))
    torch.cuda.synchronize(gpu)
    assert_same(want, sa, "after overflow, one call")
    assert_same(want, sb, "after overflow, in ranges")


@pytest.mark.parametrize("order", ["in_order", "descending", "singles"])
def test_first_frame_on_a_dirty_workspace(gpu, order):
    """The sliced counterpart of test_counters_do_not_depend_on_what_the_workspace_held_before: run (b) is the first frame
    of a workspace filled with 0xFF (counters, tile costs, strip table, records)."""
    same_frame(gpu, "base", ORDERS[order], fill=0xFF)


def test_ranges_behind_a_pending_side_stream_preparation(gpu):
    """A one-call training forward of ANOTHER view whose backward never comes leaves its backward preparation running on the
    handle's side stream; the next frame is issued in ranges right behind it (the range that starts at slice 0 joins the side
    stream), completed and differentiated: the same frame as on a fresh renderer."""
    params, cam, kw, max_pairs, g, want = reference(gpu, "base")
    other = make_camera(W, H, yaw_deg=-6.0)
    nan_params = [torch.full_like(t, float("nan")) for t in params]
    b = Frame(gpu, params, other, max_pairs, fill=0, **kw)
    assert b.f.async_, "the renderer's side-stream handle is part of the description"
    b.one_call()  # (no synchronisation, no backward)
    got = b.describe(nan_params, cam).in_ranges(ORDERS["descending"], source=params).snapshot()
    got.update(b.backward(g))
    torch.cuda.synchronize(gpu)
    assert_same(want, got, "pending preparation")


def test_out_of_order_ranges_against_the_oracle(gpu):
    """Run (b)'s image against OracleFrame with test_frame_forward_parity's comparison (tests/test_gpu_frame.py,
    check_forward: counters and sorted lists exact, image within IMG_ATOL), unchanged."""
    from test_gpu_frame import IMG_ATOL

    scene, cam, _, _ = _case_arrays("base")
    of = OracleFrame(scene, cam)
    got = same_frame(gpu, "base", ORDERS["descending"])
    v, m, o, _ = got["stats"]
    assert o == 0 and v == int(of.mask.sum()) and m == len(of.ids)
    assert np.array_equal(got["sorted_keys"].cpu().numpy().view(np.uint64), of.keys)
    assert np.array_equal(got["sorted_ids"].cpu().numpy(), of.ids)
    err = np.abs(got["image"].cpu().numpy() - of.image).max()
    assert err < IMG_ATOL, err
    assert np.abs(got["padded"].cpu().numpy() - of.padded).max() < IMG_ATOL
    print("PHASES oracle image_err %.3g" % err)


def test_repeatable(gpu):
    a = same_frame(gpu, "base", ORDERS["descending"])
    b = same_frame(gpu, "base", ORDERS["descending"])
    assert_same(a, b, "repeat")


# ----------------------------------------------------------------------------------------------------------- refusals
def _refused(rc, reason):
    assert rc == GS_E_INVALID, rc
    assert reason.encode() in _lib.gs_last_error(), _lib.gs_last_error()


def test_refused_ranges_enqueue_nothing(gpu):
    params, cam, kw, max_pairs, g, want = reference(gpu, "base")
    b = sliced_frame(gpu, "base")
    for s0, s1 in ((-1, 3), (3, 3), (5, 2), (0, 0)):  # slice_begin < 0, slice_end <= slice_begin
        _refused(b.project(s0, s1), "bad slice range")
    for s0, s1 in ((0, 80), (70, 80), (79, 80)):  # slice_end beyond the plan of 79
        _refused(b.project(s0, s1), "bad slice range")
    # nothing was projected: the frame issued now, in ranges from all-NaN buffers in a zeroed workspace, is the one-call frame
    got = b.in_ranges(ORDERS["descending"], source=params).snapshot()
    got.update(b.backward(g))
    assert_same(want, got, "after refused ranges")


def test_table_variant_frame_is_refused(gpu):
    params, cam, kw, max_pairs, g, want = reference(gpu, "base")
    t = Frame(gpu, params, cam, max_pairs, fill=0, **{**kw, "force_strips": False, "table_bin": True})
    assert t.plan() == (0, 0) and _lib.gs_frame_binning_variant(C.byref(t.f)) == 2  # "table"
    for s0, s1 in ((0, 1), (0, 79), (1, 2)):
        _refused(t.project(s0, s1), "cannot be issued in ranges")
    got = t.one_call().snapshot()  # the valid frame afterwards: every variant lists the same pairs and draws the same image
    for k in ("image", "padded", "stats", "sorted_keys", "sorted_ids"):
        assert_same({k: want[k]}, {k: got[k]}, "table variant after the refusal")


def test_partial_range_of_an_occlusion_culled_frame_is_refused(gpu):
    params, cam, kw, max_pairs, _, _ = reference(gpu, "base")
    kw = {**kw, "training": False, "emit_sorted_keys": False}
    ref = Frame(gpu, params, cam, max_pairs, **kw).one_call().snapshot_image()
    c = Frame(gpu, params, cam, max_pairs, **kw)
    c.one_call()  # an inference forward of the same size leaves the cut table the flag promises
    c.f.flags |= _lib.GS_FRAME_OCCLUSION_CULL
    culled = C.c_int32(0)
    _lib.check(_lib.gs_frame_is_occlusion_culled(C.byref(c.f), C.byref(culled)), "gs_frame_is_occlusion_culled")
    assert culled.value == 1 and c.plan() == (79, 256)
    for s0, s1 in ((0, 1), (0, 78), (1, 79), (40, 41)):
        _refused(c.project(s0, s1), "projected in one piece")
    _lib.check(c.project(0, 79), "gs_frame_forward_project")  # in one piece it is a frame like any other
    _lib.check(_lib.gs_frame_forward_rest(C.byref(c.f), _stream(gpu)), "gs_frame_forward_rest")
    assert torch.equal(_bits(c.snapshot_image()), _bits(ref))


# ------------------------------------------------------------------------------------------- FrameRenderer's phases
def _one_call(gpu, params, cam, g, **kw):
    """image, padded and the five gradients of a fresh renderer's forward + backward."""
    r = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=False, **kw)
    img, pad = r.forward(*params, cam)
    grads = r.backward(g)
    return [img.clone(), pad.clone()] + [t.clone() for t in grads], r


def _same_lists(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), (what, k)


def _trainer_like(gpu, **kw):
    return FrameRenderer(gpu, max_pairs=1 << 20, training=True, **{"auto_grow": "async", **kw})


def test_forward_begin_declines_and_issues_nothing(gpu):
    params, cam, _, _, g, _ = reference(gpu, "base")
    want, _ = _one_call(gpu, params, cam, g)
    fewer = [t[:N_BASE - 300].contiguous() for t in params]

    def declined(r, p=params, **kw):
        assert r.forward_begin(*p, cam, 0, 79, **kw) is False
        assert r._begun is None and not r.begun_frame_matches(*p, cam)
        with pytest.raises(RuntimeError):
            r.forward_finish()
        img, pad = r.forward(*params, cam)
        _same_lists(want, [img, pad] + list(r.backward(g)), "forward after a declined forward_begin")

    r = _trainer_like(gpu, auto_grow=True)  # every frame is capacity-checked synchronously: never split
    r.forward(*params, cam)
    declined(r)
    declined(_trainer_like(gpu))  # the first frame of a renderer: its capacity has not been checked
    r = _trainer_like(gpu)
    r.forward(*fewer, cam)
    declined(r)  # another Gaussian count than the last frame's
    r = _trainer_like(gpu, force_strips=False, table_bin=True)
    r.forward(*params, cam)
    assert r.binning_variant() == "table"
    declined(r)
    r = _trainer_like(gpu)
    r.forward(*params, cam)
    with pytest.warns(UserWarning, match="project slices of 512"):
        declined(r, expect_per_slice=512)
    # ... and the same renderer does begin once nothing stands in the way (behind a frame of ANOTHER view: a slice that
    # nobody projected would hold that view's records)
    r.forward(*params, make_camera(W, H, yaw_deg=-6.0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert r.forward_begin(*params, cam, 0, 79, expect_per_slice=256) is True
    _same_lists(want[:2], r.forward_finish(), "forward_finish")
    _same_lists(want[2:], r.backward(g), "backward behind forward_finish")


def test_begun_frame_matches_finish_and_abandon(gpu):
    params, cam, _, _, g, _ = reference(gpu, "base")
    want, _ = _one_call(gpu, params, cam, g)
    other = make_camera(W, H, yaw_deg=-6.0)
    r = _trainer_like(gpu)
    r.forward(*params, other)
    assert r.forward_begin(*params, cam, 0, 1) and not r.begun_frame_matches(*params, cam)
    with pytest.raises(RuntimeError, match="issued completely"):
        r.forward_finish()
    # (forward_finish dropped nothing: the frame is still open) the remaining ranges, out of order
    assert r._begun is not None
    for s0, s1 in ((38, 79), (1, 8), (8, 38)):
        assert not r.begun_frame_matches(*params, cam)
        assert r.forward_begin(*params, cam, s0, s1)
    assert r.begun_frame_matches(*params, cam)
    clones = [t.clone() for t in params]
    assert not r.begun_frame_matches(*clones, cam)  # equal values in other tensor objects
    assert not r.begun_frame_matches(*params[:4], clones[4], cam)
    assert not r.begun_frame_matches(*params, copy.copy(cam))  # an equal camera that is another object
    assert r.begun_frame_matches(*params, cam)
    _same_lists(want[:2], r.forward_finish(), "forward_finish")
    _same_lists(want[2:], r.backward(g), "backward behind forward_finish")
    assert not r.begun_frame_matches(*params, cam)
    # abandon: a half-issued frame of another view is dropped, the one-call frame follows
    assert r.forward_begin(*params, other, 0, 40)
    r.forward_abandon()
    assert r._begun is None and not r.begun_frame_matches(*params, other)
    assert r.forward_begin(*params, other, 40, 79) is False  # no frame is open: nothing to continue
    img, pad = r.forward(*params, cam)
    _same_lists(want, [img, pad] + list(r.backward(g)), "forward after forward_abandon")


@pytest.mark.parametrize("later", [True, False])
def test_backward_kernel_choice_is_the_one_at_forward_finish(gpu, later):
    """GS_FRAME_BWD_ROWS is flipped between forward_begin and forward_finish: the backward is the one-call frame's under the
    LATER setting (the two kernels differ in their last bits)."""
    params, cam, _, _, g, _ = reference(gpu, "base")
    want, ref = _one_call(gpu, params, cam, g, bwd_rows=later)
    assert bool(ref._frame.flags & _lib.GS_FRAME_BWD_ROWS) == later
    r = _trainer_like(gpu, bwd_rows=not later)
    r.forward(*params, make_camera(W, H, yaw_deg=-6.0))  # (another view: the begun frame inherits nothing of its own)
    assert bool(r._frame.flags & _lib.GS_FRAME_BWD_ROWS) != later
    for s0, s1 in ORDERS["descending"]:
        assert r.forward_begin(*params, cam, s0, s1)
    assert bool(r._begun["f"].flags & _lib.GS_FRAME_BWD_ROWS) != later
    r.bwd_rows = later
    got = list(r.forward_finish())
    assert bool(r._frame.flags & _lib.GS_FRAME_BWD_ROWS) == later
    got += list(r.backward(g))
    _same_lists(want, got, "bwd_rows flipped to %s" % later)
    other, _ = _one_call(gpu, params, cam, g, bwd_rows=not later)
    assert any(not torch.equal(x, y) for x, y in zip(want[2:], other[2:]))  # the choice is visible in the bits


# ----------------------------------------------------- Trainer: depth-supervised views under the collective path
SCHEDULE = (0, 1, 2, 1, 1, 0, 2, 1, 1, 2, 0, 1)
DEPTH_VIEWS = (0, 2)  # views 0 and 2 have range maps, view 1 has none
MISPREDICTED = 4      # the hint given at this step names the plain view 1; the step that follows renders depth view 0
HALF_BEFORE = 9       # in front of this step (depth view 2) one project slice of view 1 is issued by hand


def _hints():
    h = list(SCHEDULE[1:]) + [None]
    h[MISPREDICTED] = 1
    return h


def expected_pickups(bucketed):
    """Steps whose frame forward_finish completes: the previous step was told this view, the view is plain, and it had been
    rendered -- capacity-checked -- on this Gaussian set before the previous step issued its project stage ahead."""
    hints, out = _hints(), []
    for t in range(1, len(SCHEDULE)):
        v = SCHEDULE[t]
        if bucketed and hints[t - 1] == v and v not in DEPTH_VIEWS and v in SCHEDULE[:t]:
            out.append(t)
    return out


def test_expected_pickups_of_the_schedule():
    assert SCHEDULE[MISPREDICTED + 1] == 0 and SCHEDULE[HALF_BEFORE] == 2
    assert expected_pickups(True) == [3, 4, 7, 8, 11] and expected_pickups(False) == []


def test_trainer_depth_views_under_the_collective_path(gpu):
    """A depth-supervised Trainer with a process group up (one rank, RCCL, the collective forced): depth views run
    backward(part=GS_BWD_RASTER, grad_depth, grad_alpha) + backward_slice per exchange slice and are never projected ahead;
    plain views in between are.  Parameters, loss values, depth loss values and the densification statistic equal the
    plain run's bit for bit; the frames picked up by forward_finish are exactly those the schedule says."""
    import os

    import torch.distributed as dist

    from gs_train import TrainOptions, Trainer

    Wt, Ht = 128, 96
    scene = make_scene(3001, Wt, Ht, seed=6)
    cams = []
    for yaw, tx in ((-3.0, -0.05), (0.0, 0.0), (3.0, 0.05)):
        c = make_camera(Wt, Ht, yaw_deg=yaw)
        c.tran = np.array([tx, 0.0, 0.0], np.float32)
        cams.append(c)
    gt = to_torch(scene, gpu)
    truth = FrameRenderer(gpu, max_pairs=1 << 18, auto_grow=True)
    images, depths = [], []
    for k, cam in enumerate(cams):
        img, _, d, a = truth.forward(*gt, cam, training=False, aux=True)
        images.append(img.clone())
        depths.append(torch.where(a >= 0.5, d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous()
                      if k in DEPTH_VIEWS else None)
    start = [t.clone() for t in gt]
    start[0] = start[0] * 1.02
    start[4] = start[4] + 0.5 * torch.randn(start[4].shape, device=gpu, generator=torch.Generator(gpu).manual_seed(2))
    opt = TrainOptions(n_iters=100, n_iters_warmup=3, depth_weight=0.1, scale_reg=0.01, opa_reg=0.02)
    hints = _hints()
    runs = []
    for exchange, n_slices in ((None, 1), ("all_reduce", 1), ("all_reduce", 3), ("reduce_scatter", 3)):
        bucketed = exchange is not None
        if bucketed:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
        try:
            tr = Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 18, exchange=exchange or "all_reduce",
                         n_slices=n_slices, depths=depths)
            tr.flat.force_collective = bucketed
            assert tr.flat.n_slices == n_slices and tr.flat.project_slice == 256
            assert tr.flat.collective_active() == bucketed and tr.optimizer.sharded == (exchange == "reduce_scatter")
            r = tr.renderer
            pickups, vals, dvals, begun = [], [], [], {}
            for it, view in enumerate(SCHEDULE):
                if bucketed and it == HALF_BEFORE:
                    tr.flat.finish_gather()
                    # a half-projected plain frame in front of a depth view: one project slice of view 1, by hand
                    assert r.forward_begin(*tr.flat.params, cams[1], 0, 1, expect_per_slice=256)
                if bucketed and it in (HALF_BEFORE, MISPREDICTED + 1):
                    assert r._begun is not None and r._begun["camera"] is cams[1]
                    begun[it] = (r._begun["done"], r._begun["slices"])
                matches = r.begun_frame_matches(*tr.flat.params, cams[view])
                assert not (matches and view in DEPTH_VIEWS)
                if matches:
                    pickups.append(it)
                vals.append(tr.train_step(it, view, next_camera_id=hints[it]).clone())
                aux = bool(r._frame.flags & _lib.GS_FRAME_AUX)
                assert aux == (view in DEPTH_VIEWS)
                if aux:
                    dvals.append(tr.depth_loss.values.clone())
                    assert r._begun is None or r._begun["camera"] is not cams[view]
            assert pickups == expected_pickups(bucketed), (exchange, n_slices, pickups)
            # the depth views at these two steps found a plain frame of view 1 in the workspace -- one project slice of 12 issued
            # by hand, all 12 issued behind the previous step on a wrong hint -- and abandoned it
            assert begun == ({HALF_BEFORE: (1, 12), MISPREDICTED + 1: (12, 12)} if bucketed else {}), begun
            assert r.overflowed_frames == 0
            tr.flat.finish_gather()
            runs.append(([p.clone() for p in tr.flat.params], torch.stack(vals), torch.stack(dvals),
                         tr.optimizer.accum_grad.clone()))
            print("PHASES trainer", exchange, n_slices, "picked up at steps", pickups)
        finally:
            if bucketed:
                dist.destroy_process_group()
    for other in runs[1:]:
        for a, b in zip(runs[0][0], other[0]):
            assert torch.equal(a, b)
        for k in (1, 2, 3):
            assert torch.equal(runs[0][k], other[k]), k
    assert float((runs[0][0][0] - start[0]).abs().max()) > 0
    assert len(runs[0][2]) == sum(v in DEPTH_VIEWS for v in SCHEDULE) and float(runs[0][2][:, 0].min()) > 0
