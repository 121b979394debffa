"""GPU tier: the project stage of an occlusion-culled frame compacts per WAVE (cull_project.hip: project_cull_count_body) --
every wave keeps its survivors in a ring of its own, projects 64 of them as soon as it has 64, and the leftovers of the 16
waves are pooled at the end of the slice.  The tests walk the regimes of that scheme: a slice smaller than the workgroup, rings
that drain more than once, the product's mix, a slice without a survivor, the ranks of the staged entries, non-finite
parameters inside a draining wave.

Shapes: 320 x 240 = 20 x 15 tiles = 45 strips, the smallest Gaussian counts that reach each regime.  Every image is compared
bit for bit with a renderer with the cull off on the same inputs, with and without a scene pack; records and rectangles of the
projected Gaussians with that renderer's; counts with what the parent commit (c642b55, one survivor queue per workgroup)
reports on the GPU for the same frames (PARENT below: never taken from the tree under test)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import to_torch

pytestmark = pytest.mark.gpu

W, H, STRIPS = 320, 240, 45
PAT32, PAT64 = -0x5a5a5a5b, -0x5a5a5a5a5a5a5a5b  # 0xa5 in every byte
M64 = (1 << 64) - 1
# (pairs of the culled frame, Gaussians projected, staged entries, order-free hash of the staged entries per slice) at a static
# pose, as the parent commit reports them
PARENT = {
    "small": (38632, 10262, 20129, 11454600761646822906),
    "faint": (928589, 574421, 742436, 12852583497214935194),
    "mix": (42764, 10732, 21954, 10513327161172392722),
    "hole": (38665, 10303, 20189, 15058127199928828330),
    "nonfinite": (911280, 568876, 730675, 12379775757392135614),
}


@functools.lru_cache(maxsize=None)
def _scene(kind):
    if kind == "small":  # 183 slices of 768: waves 12 - 15 of every workgroup have no Gaussian
        s = make_scene(140_000, W, H, seed=21)
        s.opa += 3.0  # opaque: every tile's pixels stop long before the end of its list
    elif kind == "hole":  # the sixth slice lies behind the camera
        s = make_scene(140_000, W, H, seed=21)
        s.opa += 3.0
        s.pos[5 * 768:6 * 768, 2] = -np.abs(s.pos[5 * 768:6 * 768, 2]) - 1.0
    elif kind == "mix":  # 245 slices of 3,072 = 3 rounds of the workgroup
        s = make_scene(750_000, W, H, seed=25)
        s.opa += 3.0
    else:  # "faint" / "nonfinite": no tile saturates, every Gaussian that can reach a tile is projected; 245 slices of 4,096
        s = make_scene(1_000_000, W, H, seed=26, max_px_sigma=2.0)
        s.opa[:] = -7.0
        if kind == "nonfinite":
            # in waves 0 - 2 of slices 0 and 1, all four rounds
            sl, rnd, wv, ln = np.meshgrid(np.arange(2), np.arange(4), np.arange(3), np.arange(64), indexing="ij")
            idx = (4096 * sl + 1024 * rnd + 64 * wv + ln).ravel()
            idx = np.random.default_rng(9).choice(idx, size=48, replace=False).reshape(6, 8)
            s.pos[idx[0]] = np.nan
            s.pos[idx[1], 2] = np.inf
            s.scale[idx[2], 1] = np.nan  # (the pack's smax is NaN for these two)
            s.scale[idx[3], 0] = np.inf
            s.opa[idx[4]] = np.nan
            s.opa[idx[5]] = np.inf
    return s


def _nonfinite_scales():
    s = _scene("nonfinite")
    return np.flatnonzero(~np.isfinite(s.scale).all(1))


def _stage(r):
    """(entries u64 as int64, tags as int32, slice_entries [1024] as int32, slices, cap) of the renderer's last frame
    description, which must be a culled one: views of the workspace."""
    f = r._frame
    ent, tag, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    slices, cap = C.c_int32(), C.c_int64()
    _lib.check(_lib.gs_frame_debug_cull_stage(C.byref(f), C.byref(ent), C.byref(tag), C.byref(cnt), C.byref(slices),
                                              C.byref(cap)), "gs_frame_debug_cull_stage")
    base = r._ws.data_ptr()

    def view(ptr, nbytes, dtype):
        return r._ws[ptr.value - base:ptr.value - base + nbytes].view(dtype)

    return (view(ent, 8 * int(f.max_pairs), torch.int64), view(tag, 4 * int(f.max_pairs), torch.int32),
            view(cnt, 4 * 1024, torch.int32), slices.value, cap.value)


def _records(r):
    """[N, 16] int32 view of the 64-byte records of the renderer's last frame description."""
    f = r._frame
    ptrs = [C.c_void_p() for _ in range(7)]
    _lib.check(_lib.gs_frame_debug_views(C.byref(f), *[C.byref(p) for p in ptrs]), "gs_frame_debug_views")
    off = ptrs[3].value - r._ws.data_ptr()
    return r._ws[off:off + 64 * f.N].view(torch.int32).reshape(f.N, 16)


class Frame:
    """One scene at a static pose: an unculled reference frame, culled frames with and without a scene pack, and the project
    stage of the culled frame description run once more, alone, over patterned rectangles and staging."""

    def __init__(self, gpu, kind, pack, max_pairs):
        scene, cam = _scene(kind), make_camera(W, H)
        params = to_torch(scene, gpu)
        kw = dict(max_pairs=max_pairs, auto_grow=False, long_lists=False)
        r = FrameRenderer(gpu, scene_pack=None if pack else False, **kw)
        off = FrameRenderer(gpu, occlusion_cull=False, scene_pack=False, **kw)
        ref, _ = off.forward(*params, cam)
        self.full = off.stats()
        assert self.full.overflow == 0
        self.off_rects = off._rects().clone()
        self.off_rec = _records(off).clone()

        def same(a, b):
            return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))

        self.pairs = []
        for k in range(4):
            r._cull_off_until = 0  # (the adaptive policy kept out of the way)
            img, _ = r.forward(*params, cam)
            st = r.stats()
            assert bool(r._frame.flags & 256) == (k > 0) and r.binning_variant() == "strip"
            assert same(img, ref), (kind, pack, k, st)
            assert st.overflow == 0 and st.visible == self.full.visible
            if k > 0:
                self.pairs.append((st.pairs, st.cull_fallback))
        assert r.scene_pack_active() == pack
        self.n = scene.n
        ent, tag, cnt, self.slices, self.cap = _stage(r)
        self.per_slice = -(-(-(-self.n // 256)) // 256) * 256  # (gs_strip_plan_for)
        assert self.slices == -(-self.n // self.per_slice)
        rects, rec = r._rects(allow_culled=True), _records(r)
        torch.cuda.synchronize()
        rects.fill_(PAT32)
        ent.fill_(PAT64)
        tag.fill_(PAT32)
        cnt.fill_(PAT32)
        _lib.check(_lib.gs_frame_forward_project(C.byref(r._frame), 0, self.slices, torch.cuda.current_stream(gpu).cuda_stream),
                   "gs_frame_forward_project")
        torch.cuda.synchronize()
        self.written = (rects != PAT32).any(1)
        self.rects, self.rec = rects, rec
        w = self.written.cpu().numpy()
        self.w = np.concatenate([w, np.zeros(self.slices * self.per_slice - self.n, bool)]).reshape(self.slices, self.per_slice)
        self.surv = self.w.sum(1)  # Gaussians projected, per slice
        self.cnt = cnt[:self.slices].cpu().numpy().astype(np.int64) & 0xffffffff
        assert (cnt[self.slices:].cpu().numpy() == np.int32(PAT32)).all() and (self.cnt < self.cap).all()
        self.ent = ent[:self.slices * self.cap].cpu().numpy().reshape(self.slices, self.cap)
        self.tag = tag[:self.slices * self.cap].cpu().numpy().reshape(self.slices, self.cap)
        # nothing written outside a slice's own prefix
        beyond = np.arange(self.cap)[None, :] >= self.cnt[:, None]
        assert (self.ent[beyond] == np.int64(PAT64)).all() and (self.tag[beyond] == np.int32(PAT32)).all()
        h = 0
        for s in range(self.slices):  # order-free inside a slice: the entries' sum and the sum of their squares mod 2^64
            e = self.ent[s, :self.cnt[s]].astype(np.uint64)
            h = (h * 0x100000001b3 + int(e.sum(dtype=np.uint64)) + 31 * int((e * e).sum(dtype=np.uint64))) & M64
        self.figures = (self.pairs[0][0], int(self.surv.sum()), int(self.cnt.sum()), h)
        print("\ncull waves", kind, "pack" if pack else "raw", "| culled frames", self.pairs, "of", self.full.pairs, "| figures",
              self.figures, "| slices", self.slices, "x", self.per_slice, "| survivors per slice: max", int(self.surv.max()),
              "min", int(self.surv.min()), "| per wave: max", int(self.per_wave().max()))

    def per_wave(self):
        """[slices, 16]: Gaussians projected, per wave of the slice's workgroup (Gaussian i of a slice: wave (i mod 1,024) / 64)"""
        i = np.arange(self.per_slice)
        out = np.zeros((self.slices, 16), np.int64)
        for wv in range(16):
            out[:, wv] = self.w[:, (i % 1024) // 64 == wv].sum(1)
        return out

    def check_projected(self):
        """rectangles and records of the projected Gaussians: the unculled frame's, byte for byte; every Gaussian the
        unculled frame lists in a tile that the cull could not drop is among them"""
        m = self.written
        assert torch.equal(self.rects[m], self.off_rects[m])
        a, b = self.rec[m].view(torch.float32), self.off_rec[m].view(torch.float32)  # (a NaN is a NaN: payloads not compared)
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a).view(torch.int32), torch.nan_to_num(b).view(torch.int32))
        assert not (m & (self.off_rects[:, 2] == 0)).any()  # never a Gaussian outside the frustum

    def check_parent(self, kind):
        assert all(p == (self.figures[0], False) for p in self.pairs), self.pairs
        assert self.figures == PARENT[kind], (kind, self.figures)


@pytest.mark.parametrize("pack", [False, True])
def test_a_slice_smaller_than_the_workgroup(gpu, pack):
    """140,000 Gaussians: 183 slices of 768.  Waves 12 - 15 of a workgroup have nothing to test and still reach the pooled
    tail's barrier; no wave gathers 64 survivors, everything goes through the tail, which pools the leftovers of twelve waves."""
    f = Frame(gpu, "small", pack, 1 << 20)
    assert (f.slices, f.per_slice) == (183, 768)
    pw = f.per_wave()
    assert (pw[:, 12:] == 0).all() and pw[:, :12].max() < 64 and 0 < f.surv.min() and f.surv.max() < 768
    assert f.pairs[0][0] < f.full.pairs
    f.check_projected()
    f.check_parent("small")


@pytest.mark.parametrize("pack", [False, True])
def test_rings_that_drain_more_than_once(gpu, pack):
    """A faint scene: no tile saturates, every cut is GS_NO_CUT and every Gaussian that can reach a tile is projected -- more
    than 2,048 of a slice's 4,096, i.e. more than 128 per wave on average: a wave's ring goes round."""
    f = Frame(gpu, "faint", pack, 1 << 22)
    assert (f.slices, f.per_slice) == (245, 4096)
    pw = f.per_wave()
    assert f.surv.max() > 2048 and pw.max() > 128
    assert f.pairs[0][0] == f.full.pairs  # nothing to cull
    assert not ((f.off_rects[:, 3] != 0) & ~f.written).any()  # every Gaussian with a tile was projected
    f.check_projected()
    f.check_parent("faint")


@pytest.mark.parametrize("pack", [False, True])
def test_the_products_mix_and_the_ranks_of_its_staged_entries(gpu, pack):
    """The opaque scene at three rounds per workgroup.  At this frame size the cuts leave a few per cent of a slice's Gaussians
    (a wave projects up to ten of its 192: measured on the parent), so every survivor goes through the pooled tail, which is
    neither empty nor full; waves that drain in different rounds are the faint scene's.  Then the tags of the staged entries:
    for every (slice, strip) the ranks are exactly 0 .. count - 1."""
    f = Frame(gpu, "mix", pack, 6_000_000)
    assert f.per_slice >= 3 * 1024
    inside = np.minimum(f.per_slice, f.n - np.arange(f.slices) * f.per_slice)
    assert ((0 < f.surv) & (f.surv < inside)).any()
    assert 0 < np.median(f.surv) and f.surv.max() < 16 * 63  # the pooled tail: neither empty nor full
    assert f.pairs[0][0] < f.full.pairs
    f.check_projected()
    f.check_parent("mix")
    live = np.arange(f.cap)[None, :] < f.cnt[:, None]
    t = f.tag[live].astype(np.int64) & 0xffffffff
    sl = np.broadcast_to(np.arange(f.slices)[:, None], live.shape)[live]
    strip, rank = t & 8191, t >> 13
    assert (strip < STRIPS).all()
    key = sl * STRIPS + strip
    order = np.lexsort((rank, key))
    key, rank = key[order], rank[order]
    first = np.r_[True, key[1:] != key[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(key)), 0))
    assert (rank == np.arange(len(key)) - start).all()


@pytest.mark.parametrize("pack", [False, True])
def test_a_slice_without_a_survivor(gpu, pack):
    """The 768 Gaussians of the sixth slice lie behind the camera: nothing in any ring, nothing pooled, no entry staged."""
    f = Frame(gpu, "hole", pack, 1 << 20)
    assert f.surv[5] == 0 and f.cnt[5] == 0 and f.surv[4] > 0 and f.surv[6] > 0
    f.check_projected()
    f.check_parent("hole")


@pytest.mark.parametrize("pack", [False, True])
def test_non_finite_parameters_inside_a_draining_wave(gpu, pack):
    """NaN / infinite positions, scales (the pack's smax is NaN then) and opacities in the first waves of two slices of the faint
    scene, whose waves all drain: a Gaussian with a non-finite scale is not tested against the cuts but projected."""
    f = Frame(gpu, "nonfinite", pack, 1 << 22)
    idx = _nonfinite_scales()
    seen = idx[(f.off_rects[torch.from_numpy(idx).to(gpu), 2] != 0).cpu().numpy()]  # inside the frustum
    assert len(seen) > 0 and f.written[torch.from_numpy(seen).to(gpu)].all()
    pw = f.per_wave()
    assert (pw[seen // f.per_slice, (seen % f.per_slice % 1024) // 64] >= 64).all()
    f.check_projected()
    f.check_parent("nonfinite")
