"""GPU tier: the first pass of an occlusion-culled frame keeps the level-1 entries its project stage counts (entry + strip +
rank in the slice's run of the strip, staged per slice of the Gaussian array) and places them with a permutation instead of
walking every survivor's rectangle a second time (cull_project.hip: frame_project_cull_count_kernel; strip_bin.hip:
strip_scatter_kernel<false, true>).

Shapes: the smallest at which the path is the product's own -- 140 k Gaussians (the strip variant starts at 131,072: 183
slices of 768), 320 x 240 = 20 x 15 tiles = 3 strips per tile row, one of them ragged, 45 strips.  Every comparison is bit
for bit against a renderer with the cull off on the same inputs."""
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

N, W, H = 140_000, 320, 240
MAX_PAIRS = 1 << 20
# stats().pairs of the culled frames of `_opaque(N, w, h)` at a static pose, as the parent commit (97a22b9, which walked the
# survivors' rectangles twice) reports them on the GPU: the trimmed lists are the same lists
PARENT_PAIRS = {(320, 240): 38632, (300, 232): 36618}


@functools.lru_cache(maxsize=None)
def _opaque(n=N, w=W, h=H, seed=21):
    scene = make_scene(n, w, h, seed=seed)
    scene.opa += 3.0  # opaque: every tile's pixels stop long before the end of its list
    return scene


def _pair(gpu, **kw):
    kw = dict(max_pairs=MAX_PAIRS, auto_grow=False, **kw)
    return FrameRenderer(gpu, **kw), FrameRenderer(gpu, occlusion_cull=False, **kw)


def _forward(r, params, cam):
    r._cull_off_until = 0  # (the adaptive policy kept out of the way: which frames are culled does not depend on timing)
    img, _ = r.forward(*params, cam)
    return img, r.stats()


def _stage(r):
    """(entries [slices, cap] u64 as int64, tags [slices, cap] as int32, slice_entries [1024] as int32, slices, cap, and the
    flat views behind the regions) of the renderer's last frame description, which must be a culled one."""
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


def _static_pose(gpu, w, h):
    scene, cam = _opaque(N, w, h), make_camera(w, h)
    params = to_torch(scene, gpu)
    r, off = _pair(gpu)
    ref, _ = off.forward(*params, cam)
    full = off.stats().pairs
    first, st0 = _forward(r, params, cam)
    assert not (r._frame.flags & 256) and st0.pairs == full and torch.equal(first, ref)
    pairs = []
    for _ in range(4):
        img, st = _forward(r, params, cam)
        assert r._frame.flags & 256 and r.binning_variant() == "strip"
        assert not st.cull_fallback and st.overflow == 0 and st.visible == st0.visible
        assert torch.equal(img, ref)
        pairs.append(st.pairs)
        _, _, cnt, slices, cap = _stage(r)
        cnt = cnt[:slices].cpu().numpy().astype(np.int64) & 0xffffffff
        assert slices == 183 and cap == MAX_PAIRS // 183
        assert cnt.max() < cap and 0 < cnt.sum() <= st.pairs  # an entry lists at least one pair
    print("culled pairs", (w, h), pairs, "of", full)
    assert pairs == [PARENT_PAIRS[(w, h)]] * 4, (pairs, full)


def test_static_pose_is_exact_and_lists_what_the_parent_listed(gpu):
    _static_pose(gpu, W, H)


def test_ragged_grid_is_exact_and_lists_what_the_parent_listed(gpu):
    """300 x 232: 19 x 15 tiles -- the last strip of a row has three tiles, the cut rows are padded to whole strips -- and a
    height that is no multiple of 16 pixels (the padded frame is cropped)."""
    _static_pose(gpu, 300, 232)


def test_dilated_cuts_over_a_slow_pan(gpu):
    """A 0.25-px-per-frame pan: the host's rule culls every frame with the 3 x 3 dilated cuts (GS_FRAME_CULL_DILATE, the
    near factor).  Exact whether a frame's trimmed lists sufficed or not; most frames must not need the second pass."""
    params = to_torch(_opaque(), gpu)
    r, off = _pair(gpu)
    step = np.degrees(0.25 / (0.75 * W))
    dilated = clean = 0
    for k in range(20):
        cam = make_camera(W, H, yaw_deg=k * step)
        img, st = _forward(r, params, cam)
        ref, _ = off.forward(*params, cam)
        assert torch.equal(img, ref), (k, st)
        assert bool(r._frame.flags & 256) == (k > 0)
        dilated += int(bool(r._frame.flags & 512))
        clean += int(bool(r._frame.flags & 256) and not st.cull_fallback and st.pairs < off.stats().pairs)
    print("dilated", dilated, "clean", clean)
    assert dilated == 19 and clean >= 1, (dilated, clean)


def test_a_slice_beyond_its_staging_region_falls_back_and_writes_nothing_outside(gpu):
    """The last slice of the Gaussian array (300 Gaussians) is faint, in front of everything and covers the image: 45 entries
    each, 13,500 in all, against a staging region of max_pairs / slices = 5,729.  The slice stores what fits, publishes no
    entry, the frame is rendered again from the full lists (cull_fallback) and equals the unculled image.  Then the project
    stage alone is run once more over a staging area filled with a pattern: every slot outside a slice's own written prefix,
    and everything behind the last region, still holds the pattern."""
    n_front, slices, per_slice = 300, 183, 768
    n = (slices - 1) * per_slice + n_front
    base = make_scene(n, W, H, seed=22)
    base.opa += 3.0
    rng = np.random.default_rng(5)
    base.pos[-n_front:] = np.concatenate([rng.uniform(-0.01, 0.01, (n_front, 2)), np.full((n_front, 1), 0.4)], 1)
    base.scale[-n_front:] = 5.0  # a sigma of thousands of pixels
    base.opa[-n_front:] = -8.0   # 300 x 3.4e-4: the pixels stay alive behind them
    params = to_torch(base, gpu)
    cam = make_camera(W, H)
    r, off = _pair(gpu)
    ref, _ = off.forward(*params, cam)
    first, _ = _forward(r, params, cam)
    assert torch.equal(first, ref)
    img, st = _forward(r, params, cam)
    assert r._frame.flags & 256 and st.cull_fallback and st.pairs == off.stats().pairs
    assert torch.equal(img, ref)
    ent, tag, cnt, got_slices, cap = _stage(r)
    strips = 3 * 15
    assert got_slices == slices and cap == MAX_PAIRS // slices == 5729 and n_front * strips > cap
    # the project stage of the same (culled) frame description, alone, over a patterned staging area
    torch.cuda.synchronize()
    ent.fill_(-0x5a5a5a5a5a5a5a5b)  # 0xa5 in every byte
    tag.fill_(-0x5a5a5a5b)
    cnt.fill_(-0x5a5a5a5b)
    _lib.check(_lib.gs_frame_forward_project(C.byref(r._frame), 0, slices, torch.cuda.current_stream(gpu).cuda_stream),
               "gs_frame_forward_project")
    torch.cuda.synchronize()
    ent, tag, cnt = ent.cpu().numpy(), tag.cpu().numpy(), cnt.cpu().numpy()
    E_PAT, T_PAT = np.int64(-0x5a5a5a5a5a5a5a5b), np.int32(-0x5a5a5a5b)
    assert (cnt[slices:] == T_PAT).all()
    counts = cnt[:slices].astype(np.int64) & 0xffffffff
    assert counts[-1] == 0xffffffff and (counts[:-1] < cap).all() and counts[:-1].sum() > 0
    written = np.minimum(counts, cap)
    for s in range(slices):
        lo, mid, hi = s * cap, s * cap + written[s], (s + 1) * cap
        assert (tag[mid:hi] == T_PAT).all() and (ent[mid:hi] == E_PAT).all(), s
        t = tag[lo:mid].astype(np.int64) & 0xffffffff
        assert ((t & 8191) < strips).all() and ((t >> 13) < per_slice).all(), s  # (never the pattern: its strip is 1,445)
    assert (tag[slices * cap:] == T_PAT).all() and (ent[slices * cap:] == E_PAT).all()


def test_workspace_filled_with_ff_and_changes_of_the_gaussian_count(gpu):
    """Nothing the staged path reads is left over from before: a workspace handed over filled with 0xFF, then -- in the same
    workspace -- other Gaussian counts, smaller and larger (other slices, other staging regions, the previous scene's cuts)."""
    cam = make_camera(W, H)
    r, off = _pair(gpu)
    big = to_torch(_opaque(200_000, seed=23), gpu)
    off.forward(*big, cam)
    r._ws = torch.full((off._ws.numel() + (1 << 20),), 0xFF, dtype=torch.uint8, device=gpu)
    culled = clean = 0
    for params in (big, to_torch(_opaque(), gpu), to_torch(_opaque(60_000, seed=24), gpu), big):
        for k in range(3):
            img, st = _forward(r, params, cam)
            ref, _ = off.forward(*params, cam)
            assert torch.equal(img, ref), (params[0].shape[0], k, st)
            culled += int(bool(r._frame.flags & 256))
            clean += int(bool(r._frame.flags & 256) and not st.cull_fallback)
        assert not st.cull_fallback and st.pairs < off.stats().pairs  # at rest on a scene, the cull holds
    assert culled == 11 and clean >= 8, (culled, clean)


def test_non_finite_gaussians(gpu):
    """NaN / infinite positions, scales and opacities in a handful of Gaussians: equal to the unculled renderer, NaN pixels
    included."""
    src = _opaque()
    scene = type(src)(src.pos.copy(), src.quat.copy(), src.scale.copy(), src.opa.copy(), src.rgb.copy())
    idx = np.random.default_rng(9).choice(N, size=6 * 8, replace=False).reshape(6, 8)
    scene.pos[idx[0]] = np.nan
    scene.pos[idx[1], 2] = np.inf
    scene.scale[idx[2], 1] = np.nan
    scene.scale[idx[3], 0] = np.inf
    scene.opa[idx[4]] = np.nan
    scene.opa[idx[5][:4]] = np.inf
    scene.opa[idx[5][4:]] = -np.inf
    params = to_torch(scene, gpu)
    cam = make_camera(W, H)
    r, off = _pair(gpu)
    ref, _ = off.forward(*params, cam)
    culled = 0
    for k in range(4):
        img, st = _forward(r, params, cam)
        assert st.overflow == 0
        assert torch.equal(torch.isnan(img), torch.isnan(ref)), (k, st)
        assert torch.equal(torch.nan_to_num(img), torch.nan_to_num(ref)), (k, st)
        culled += int(bool(r._frame.flags & 256))
    assert culled == 3
