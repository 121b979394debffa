"""GPU tier: an occlusion-culled frame (GS_FRAME_OCCLUSION_CULL) equals the unculled frame bit for bit when the SCENE changed
under a cut table that stayed -- in-place edits of the parameter tensors, which the host does not see.

A trimmed tile list is the prefix {depth <= cut} plus the interior extras of runs that kept their ends (strip_common.h,
walk_strips<CUT>).  tests/cull_trim_ref.py models that rule on the CPU and tests/test_cull_trim_host.py pins what its crafted
scene does: after the occluder fades (or leaves), tile (3, 3) composites the wall without the three small Gaussians in front of
it, saturates there, and no tile ends live.  A fallback that only looks for live ends returns that image (wrong by 0.93 in
tile (3, 3)); the compositing kernel therefore also raises the fallback when the last Gaussian a tile composited lies behind
its cut.

Every comparison is ``torch.equal`` against a renderer with the cull off on the same tensors.  256 x 96 = 16 x 6 tiles, two
strips per tile row; 19 Gaussians (the strip plan takes any count: one slice of 256)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cull_trim_ref import OCC, SMALL_PX, crafted_camera, crafted_scene
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import C0, Scene, make_camera, make_scene
from gs_testutil import to_torch

pytestmark = pytest.mark.gpu

CULL, DILATE, NEAR = _lib.GS_FRAME_OCCLUSION_CULL, _lib.GS_FRAME_CULL_DILATE, _lib.GS_FRAME_CULL_DILATE_NEAR
MAX_PAIRS = 4096  # (the crafted scene has 1,299 pairs)


def _pair(gpu, scene_pack=True, max_pairs=MAX_PAIRS):
    kw = dict(force_strips=True, auto_grow=False, max_pairs=max_pairs, scene_pack=None if scene_pack else False)
    return FrameRenderer(gpu, **kw), FrameRenderer(gpu, occlusion_cull=False, **kw)


def _forward(r, params, cam, aux=False):
    """-> ((image,) or (image, depth, alpha), stats)"""
    r._cull_off_until = 0  # (the adaptive policy kept out of the way: which frames are culled does not depend on timing)
    out = r.forward(*params, cam, aux=aux)
    return ((out[0], out[2], out[3]) if aux else (out[0],)), r.stats()


def _is_culled(r):
    culled = C.c_int32()
    _lib.check(_lib.gs_frame_is_occlusion_culled(C.byref(r._frame), C.byref(culled)), "gs_frame_is_occlusion_culled")
    return bool(culled.value)


def _same(got, ref):
    return all(torch.equal(a, b) for a, b in zip(got, ref))


def _crafted_params(gpu, color_dim=3, wall=True):
    scene = crafted_scene(wall)
    if color_dim == 27:  # the same geometry, DC-only SH coefficients: sigmoid(C0 x logit / C0), the same colours
        sh = np.zeros((scene.n, 3, 9), np.float32)
        sh[:, :, 0] = scene.rgb / np.float32(C0)
        scene = Scene(scene.pos, scene.quat, scene.scale, scene.opa, sh.reshape(scene.n, 27))
    return to_torch(scene, gpu)


def _edit(params, how):
    pos, _, _, opa, _ = params
    with torch.no_grad():  # in place: the same tensors, so the renderer's scene key and cut key survive
        if how == "fade":
            opa[OCC] = -8.0
        else:  # "move": the occluder leaves the frustum
            pos[OCC, 0] += 100.0


def _sequence(gpu, how="fade", shift_px=0.0, scene_pack=True, color_dim=3, aux=False, wall=True):
    """Frames 1, 2 (culled, three pairs trimmed), the edit, frame 3 (must be exact: the second pass), frame 4 (culled again)."""
    params = _crafted_params(gpu, color_dim, wall)
    r, off = _pair(gpu, scene_pack)
    cam0, cam1 = crafted_camera(), crafted_camera(shift_px)
    tag = (how, shift_px, scene_pack, color_dim, aux, wall)

    ref, st_off = _forward(off, params, cam0, aux)
    full = st_off.pairs
    assert full == (1299 if wall else 1299 - 8 * 96)
    got, st = _forward(r, params, cam0, aux)
    assert not (r._frame.flags & CULL) and st.pairs == full and _same(got, ref), tag
    got, st = _forward(r, params, cam0, aux)
    assert r._frame.flags & CULL and not (r._frame.flags & DILATE) and _is_culled(r) and r.binning_variant() == "strip", tag
    assert not st.cull_fallback and st.pairs == full - 3 and st.overflow == 0, (tag, st)  # the small Gaussians' three pairs
    assert _same(got, ref), tag
    assert not (r.scene_pack_active() and not scene_pack) and (r.scene_pack_active() or not scene_pack or aux), tag

    _edit(params, how)
    ref, st_off = _forward(off, params, cam1, aux)
    full = st_off.pairs
    got, st = _forward(r, params, cam1, aux)
    want = 0 if shift_px == 0.0 else (DILATE | NEAR if shift_px <= 0.5 else DILATE)
    assert r._frame.flags & CULL and _is_culled(r) and (r._frame.flags & (DILATE | NEAR)) == want, (tag, r._frame.flags)
    diff = (got[0] - ref[0]).abs().amax(dim=2)
    print("frame 3", tag, "fallback", st.cull_fallback, "pairs", st.pairs, "of", full, "| max |culled - unculled|",
          float(diff.max()), "in", int((diff > 0).sum()), "pixels, tile (3, 3):", float(diff[48:64, 48:64].max()))
    assert _same(got, ref), (tag, "frame 3: the culled frame differs from the unculled one", float(diff.max()))
    assert st.cull_fallback and st.pairs == full, (tag, st)  # rendered again from the full lists; the counters are that pass's
    assert float(ref[0][SMALL_PX[1], SMALL_PX[0], 0]) > 0.9  # the small Gaussians are what the frame shows there

    ref, _ = _forward(off, params, cam1, aux)
    got, st = _forward(r, params, cam1, aux)
    assert r._frame.flags & CULL and not (r._frame.flags & DILATE) and _is_culled(r), tag
    assert not st.cull_fallback and st.overflow == 0 and _same(got, ref), (tag, st)  # the second pass left a valid cut table
    assert float(got[0][SMALL_PX[1], SMALL_PX[0], 0]) > 0.9


def test_faded_occluder_at_a_resting_pose(gpu):
    """The base sequence.  Without the depth test in the compositing kernel's epilogue, frame 3 fails its `torch.equal`: max
    |culled - unculled| = 0.93 in tile (3, 3), no fallback."""
    _sequence(gpu)


@pytest.mark.parametrize("shift_px", [0.0, 0.3, 2.0])
def test_occluder_moved_out_of_the_frustum(gpu, shift_px):
    _sequence(gpu, how="move", shift_px=shift_px)


@pytest.mark.parametrize("shift_px", [0.3, 2.0])
def test_edit_together_with_a_small_yaw_takes_the_dilated_cuts(gpu, shift_px):
    """0.3 px: GS_FRAME_CULL_DILATE | GS_FRAME_CULL_DILATE_NEAR (the 3 x 3 maximum x 1.125 = 2.56 at tile (3, 3)); 2 px: DILATE
    alone (x 1.375 = 3.13): both in front of the small Gaussians at 4.28 (test_cull_trim_host.py)."""
    _sequence(gpu, shift_px=shift_px)


@pytest.mark.parametrize("scene_pack", [True, False])
@pytest.mark.parametrize("color_dim", [3, 27])
def test_scene_pack_and_sh_colours(gpu, scene_pack, color_dim):
    """The packed and the raw project kernels; raster_forward_kernel<27, ...> (a liveness test every 4 Gaussians)."""
    _sequence(gpu, scene_pack=scene_pack, color_dim=color_dim)


@pytest.mark.parametrize("color_dim", [3, 27])
def test_aux_inference_frame(gpu, color_dim):
    """GS_FRAME_AUX with depth and alpha maps requested: raster_aux_forward_kernel<CD, false> shares the epilogue."""
    _sequence(gpu, color_dim=color_dim, aux=True)


def test_control_without_the_wall(gpu):
    """The block's tiles end live on their trimmed lists: the rule the kernel always had."""
    _sequence(gpu, wall=False)


def test_static_pose_never_falls_back(gpu):
    """Six culled frames of the unchanged scene: a tile at an unchanged pose stops at the Gaussian that set its cut, so the
    depth test must never fire.  Against a fix that falls back too often."""
    params = _crafted_params(gpu)
    r, off = _pair(gpu)
    cam = crafted_camera()
    ref, st_off = _forward(off, params, cam)
    got, _ = _forward(r, params, cam)
    assert _same(got, ref)
    pairs = []
    for k in range(6):
        got, st = _forward(r, params, cam)
        assert r._frame.flags & CULL and _is_culled(r) and not st.cull_fallback and _same(got, ref), (k, st)
        pairs.append(st.pairs)
    assert pairs == [st_off.pairs - 3] * 6, pairs


@pytest.mark.parametrize("seed", [41, 42])
def test_random_edits_with_large_footprints(gpu, seed):
    """6,000 opaque Gaussians with pixel sigmas up to 64 (runs that cross whole strips, so trimmed interior tiles are the rule),
    edited in place between frames: opacities swapped between two random tenths, or the nearest 2 % pushed behind the camera;
    a 0.3 degree yaw every third frame.  Every frame after the first is culled, and every frame is exact."""
    w, h = 256, 192
    scene = make_scene(6000, w, h, seed, max_px_sigma=64)
    scene.opa += 3.0
    params = to_torch(scene, gpu)
    pos, _, _, opa, _ = params
    r, off = _pair(gpu, max_pairs=1 << 20)
    r.CULL_MAX_SHIFT_PX = float("inf")
    rng = np.random.default_rng(seed)
    n, yaw, fell = scene.n, 0.0, []
    for k in range(12):
        if k:
            with torch.no_grad():
                if rng.random() < 0.5:
                    a, b = (torch.from_numpy(rng.choice(n, n // 10, replace=False)).to(gpu) for _ in range(2))
                    va, vb = opa[a].clone(), opa[b].clone()
                    opa[a] = vb
                    opa[b] = va
                else:
                    z = pos[:, 2].cpu().numpy()
                    front = np.nonzero(z > 0)[0]
                    near = front[np.argsort(z[front], kind="stable")[:n // 50]]
                    pos[torch.from_numpy(near).to(gpu), 2] = -1.0
            if k % 3 == 0:
                yaw += 0.3
        cam = make_camera(w, h, yaw_deg=yaw)
        ref, st_off = _forward(off, params, cam)
        got, st = _forward(r, params, cam)
        assert st.overflow == 0 and st_off.overflow == 0
        assert bool(r._frame.flags & CULL) == (k > 0), k
        assert _same(got, ref), (seed, k, st, float((got[0] - ref[0]).abs().max()))
        fell.append(int(st.cull_fallback))
        print("seed", seed, "frame", k, "yaw", round(yaw, 1), "culled library-side", _is_culled(r), "fallback", st.cull_fallback,
              "pairs", st.pairs, "of", st_off.pairs)
    print("seed", seed, "fallbacks per frame", fell)
