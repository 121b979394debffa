"""GPU tier of the depth / alpha maps (GS_FRAME_AUX, include/gs_abi.h; FrameRenderer.forward(aux=True) / render_aux).

The yardstick is the oracle with the two maps posed as colours: oracle.draw with the sorted colours (d_i, 1, 0), d_i =
s_pos[:, 2] = |p_c| (the sort key), gives the padded (D, A); oracle.draw_backward with those colours and the gradient
(g_D, g_A, 0) gives their rows, whose per-Gaussian colour-0 sum is dL/dd_i and enters d_pos_i[:, 2] of the same
global_culling_backward chain as the image's gradient.  Standards: the image test's abs 5e-5, scaled by the depth range for
the depth map; gradients by tests/gs_testutil.assert_grads_close.
"""
import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import (OracleFrame, assert_grads_close, aux_case, aux_colours, robust_aux_grads,  # noqa: F401
                         to_torch)

pytestmark = pytest.mark.gpu

IMG_ATOL = 5e-5


case = aux_case  # (the scene of every aux test; tests/test_gpu_pose.py imports it from here)


def oracle_aux(of):
    """Padded [padH, padW, 3]: (D, A, 0)."""
    return of.aux_maps()


def check_maps(of, depth, alpha, aux_padded=None):
    ref = oracle_aux(of)
    g = of.grid
    dscale = max(1.0, float(np.abs(of.s_pos[:, 2]).max())) if len(of.ids) else 1.0
    d, a = depth.cpu().numpy(), alpha.cpu().numpy()
    assert d.shape == (g.height, g.width) and a.shape == (g.height, g.width)
    assert np.abs(a - g.crop(ref[:, :, 1:2])[:, :, 0]).max() < IMG_ATOL
    assert np.abs(d - g.crop(ref[:, :, 0:1])[:, :, 0]).max() < IMG_ATOL * dscale
    if aux_padded is not None:
        p = aux_padded.cpu().numpy()
        assert np.abs(p[:, :, 1] - ref[:, :, 1]).max() < IMG_ATOL
        assert np.abs(p[:, :, 0] - ref[:, :, 0]).max() < IMG_ATOL * dscale
    return ref


@pytest.mark.parametrize("use_sh,deg", [(False, 2), (True, 2), (True, 3)])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("sort_mode", [0, 1, 2])
def test_aux_forward_parity(gpu, use_sh, deg, training, sort_mode):
    scene, cam = case(6000, 160, 112, seed=3, use_sh=use_sh, sh_degree=deg)
    of = OracleFrame(scene, cam)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=training, auto_grow=False, sort_mode=sort_mode)
    params = to_torch(scene, gpu)
    image, padded, depth, alpha = r.forward(*params, cam, aux=True)
    assert r._frame.flags & _lib.GS_FRAME_AUX
    assert r.stats().pairs == len(of.ids)
    assert np.abs(image.cpu().numpy() - of.image).max() < IMG_ATOL
    check_maps(of, depth, alpha, r._aux_keep[2] if training else None)
    # expected depth lies inside the scene's depth range where the pixel is covered
    cov = alpha.cpu().numpy() > 0.5
    if cov.any():
        ed = (depth.cpu().numpy() / alpha.cpu().numpy())[cov]
        assert ed.min() >= of.s_pos[:, 2].min() * 0.999 and ed.max() <= of.s_pos[:, 2].max() * 1.001


@pytest.mark.parametrize("training", [False, True])
def test_aux_forward_long_lists(gpu, training):
    """Lists beyond 2,048 pairs (the per-tile sort's LDS window) with the long-list flags on: the aux frame walks them with
    one wave (no segments) and matches the oracle to the image standard."""
    scene, cam = make_scene(120_000, 128, 96, seed=8, max_px_sigma=40.0), make_camera(128, 96)
    of = OracleFrame(scene, cam)
    assert np.diff(of.accum).max() > 2048
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=training, auto_grow=False, long_lists=True)
    image, padded, depth, alpha = r.forward(*params, cam, aux=True)
    # the aux frame composites without segments: the image standard holds (1e-3 until the errors were measured on an MI355X,
    # inference and training frame alike: image 3.6e-7, alpha 6.0e-7, depth 2.1e-7 absolute at a depth scale of 13.9)
    assert np.abs(image.cpu().numpy() - of.image).max() < IMG_ATOL
    ref = oracle_aux(of)
    g = of.grid
    assert np.abs(alpha.cpu().numpy() - g.crop(ref[:, :, 1:2])[:, :, 0]).max() < IMG_ATOL
    dscale = float(np.abs(of.s_pos[:, 2]).max())
    assert np.abs(depth.cpu().numpy() - g.crop(ref[:, :, 0:1])[:, :, 0]).max() < IMG_ATOL * dscale


@pytest.mark.parametrize("training", [False, True])
def test_alpha_is_bit_identical_to_a_white_image(gpu, training):
    """rgb logits of +30: every colour is exactly 1.0f, so each image channel is accumulated exactly as alpha is."""
    scene, cam = case(8000, 128, 96, seed=5)
    scene.rgb[:] = 30.0
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=training, auto_grow=True)
    image, padded, _, alpha = r.forward(*params, cam, aux=True)
    assert float(alpha.max()) > 0.9
    if training:
        aux_padded = r._aux_keep[2]
        for c in range(3):
            assert torch.equal(padded[:, :, c], aux_padded[:, :, 1])
        g = r._grid
        top, left = g.crop_offsets()
        assert torch.equal(alpha, aux_padded[top:top + g.height, left:left + g.width, 1])
    below = alpha <= 1.0  # (the image is clamped to [0, 1], the map is not)
    assert bool(below.all()) or float(alpha.max()) < 1.0 + 1e-6
    for c in range(3):
        assert torch.equal(image[:, :, c][below], alpha[below])


@pytest.mark.parametrize("use_sh,deg", [(False, 2), (True, 2), (True, 3)])
def test_aux_frame_image_is_unchanged(gpu, use_sh, deg):
    scene, cam = case(6000, 160, 112, seed=11, use_sh=use_sh, sh_degree=deg)
    params = to_torch(scene, gpu)
    for training in (False, True):
        r = FrameRenderer(gpu, max_pairs=1 << 18, training=training, auto_grow=True, occlusion_cull=False)
        img0, pad0 = r.forward(*params, cam)
        img1, pad1, _, _ = r.forward(*params, cam, aux=True)
        assert torch.equal(img0, img1)
        if training:
            assert torch.equal(pad0, pad1)


def _dense(seed=3):
    scene = make_scene(60_000, 192, 128, seed=seed)
    scene.opa += 3.0  # opaque: every tile's pixels stop long before the end of its list (what the cull trims)
    return scene, make_camera(192, 128)


def test_cull_alternating_plain_and_aux_frames_is_bit_exact(gpu):
    scene, cam = _dense()
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False, occlusion_cull=False)
    ref_img, _, ref_d, ref_a = off.forward(*params, cam, aux=True)
    culled = 0
    for k in range(6):
        aux = k % 2 == 1
        out = r.forward(*params, cam, aux=aux)
        st = r.stats()
        culled += bool(r._frame.flags & _lib.GS_FRAME_OCCLUSION_CULL)
        assert not st.cull_fallback
        assert torch.equal(out[0], ref_img)
        if aux:
            assert torch.equal(out[2], ref_d) and torch.equal(out[3], ref_a)
    assert culled >= 4


def test_cull_moving_camera_gated_second_pass_keeps_maps_exact(gpu):
    """Every frame culled by the previous frame's cuts (the policy lifted); the jumps make tiles run past their cuts and
    the gated second pass render the frame again: depth and alpha stay bit-identical to the unculled renderer's."""
    scene, _ = _dense(seed=5)
    params = to_torch(scene, gpu)
    off = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False, occlusion_cull=False)
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
    r.CULL_MAX_SHIFT_PX = float("inf")
    fell = culled = 0
    for k, yaw in enumerate([0.0, 0.0, 4.0, 4.0, 30.0, -20.0, 0.0]):
        cam = make_camera(192, 128, yaw_deg=yaw)
        r._cull_off_until = 0  # (the adaptive switch kept out of the way: a fallback would switch the cull off)
        img, _, d, a = r.forward(*params, cam, aux=True)
        st = r.stats()
        culled += bool(r._frame.flags & _lib.GS_FRAME_OCCLUSION_CULL)
        fell += bool(st.cull_fallback)
        ri, _, rd, ra = off.forward(*params, cam, aux=True)
        assert torch.equal(img, ri) and torch.equal(d, rd) and torch.equal(a, ra), (k, yaw)
    assert culled >= 5 and fell >= 1, (culled, fell)


def _aux_reference(of, gimg, gd, ga):
    """The oracle's gradient of <gimg, image> + <gd, depth> + <ga, alpha> and its conditioning scale."""
    return of.aux_backward(gimg, gd, ga, with_scale=True)


def _random_grads(of, seed, image=True):
    return robust_aux_grads(of, seed, image=image)[:3]


@pytest.mark.parametrize("use_sh,deg", [(False, 2), (True, 2), (True, 3)])
@pytest.mark.parametrize("with_image", [False, True])
def test_aux_gradients_match_oracle(gpu, use_sh, deg, with_image):
    scene, cam = case(5000, 128, 96, seed=13, use_sh=use_sh, sh_degree=deg)
    of = OracleFrame(scene, cam)
    gimg, gd, ga = _random_grads(of, 17, image=with_image)
    ref, scale = _aux_reference(of, gimg, gd, ga)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    params = to_torch(scene, gpu)
    r.forward(*params, cam, aux=True)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    grads = r.backward(t(gimg), grad_depth=t(gd), grad_alpha=t(ga))
    got = [x.cpu().numpy() for x in grads]
    assert_grads_close(got, ref, scale, f"aux sh={use_sh} deg={deg} image={with_image}")
    culled = ~of.mask.astype(bool)
    for x in got:
        assert np.all(x[culled] == 0)


@pytest.mark.parametrize("use_sh,deg", [(False, 2), (True, 2), (True, 3)])
def test_aux_backward_in_parts_and_repeatable(gpu, use_sh, deg):
    scene, cam = case(20_000, 160, 112, seed=19, use_sh=use_sh, sh_degree=deg)
    of = OracleFrame(scene, cam)
    gimg, gd, ga = _random_grads(of, 23)
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    params = to_torch(scene, gpu)
    r.forward(*params, cam, aux=True)
    full = [x.clone() for x in r.backward(t(gimg), grad_depth=t(gd), grad_alpha=t(ga))]
    again = r.backward(t(gimg), grad_depth=t(gd), grad_alpha=t(ga))
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    out = tuple(torch.full_like(x, float("nan")) for x in full)
    r.backward(t(gimg), out=out, part=_lib.GS_BWD_RASTER, grad_depth=t(gd), grad_alpha=t(ga))
    n = scene.n
    for b0 in range(0, n, 4096):
        r.backward_slice(out, b0, min(b0 + 4096, n))
    for a, b in zip(full, out):
        assert torch.equal(a, b)
    out2 = tuple(torch.full_like(x, float("nan")) for x in full)
    r.backward(t(gimg), out=out2, part=_lib.GS_BWD_RASTER, grad_depth=t(gd), grad_alpha=t(ga))
    r.backward(None, out=out2, part=_lib.GS_BWD_COLOR)
    r.backward(None, out=out2, part=_lib.GS_BWD_GEOMETRY)
    for a, b in zip(full, out2):
        assert torch.equal(a, b)


def test_render_aux_autograd(gpu):
    scene, cam = case(5000, 128, 96, seed=29)
    of = OracleFrame(scene, cam)
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    image, depth, alpha = r.render_aux(*params, cam)
    assert image.shape == (96, 128, 3) and depth.shape == (96, 128) and alpha.shape == (96, 128)
    (depth / alpha.clamp_min(1e-6)).mean().backward()
    got = [p.grad.clone() for p in params]
    assert any(float(g.abs().max()) > 0 for g in got)
    # the explicit chain: the same frame, dL/dD = 1 / (A' HW), dL/dA = -D / (A'^2 HW) where A > 1e-6 (else A' = 1e-6 and
    # the clamp passes no gradient to A)
    d, a = depth.detach(), alpha.detach()
    hw = float(d.numel())
    ac = a.clamp_min(1e-6)
    gd = (1.0 / ac) / hw
    ga = torch.where(a >= 1e-6, -d / (ac * ac) / hw, torch.zeros_like(a))
    p2 = to_torch(scene, gpu)
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
    r2.forward(*p2, cam, aux=True)
    ref = r2.backward(None, grad_depth=gd.contiguous(), grad_alpha=ga.contiguous())
    for x, y in zip(got, ref):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-6 * float(y.abs().max() + 1e-30))
    # an image-only loss through render_aux equals render()'s gradient
    p3 = to_torch(scene, gpu, requires_grad=True)
    img3, _, _ = r.render_aux(*p3, cam)
    img3.sum().backward()
    p4 = to_torch(scene, gpu, requires_grad=True)
    r.render(*p4, cam).sum().backward()
    for x, y in zip(p3, p4):
        assert torch.allclose(x.grad, y.grad, rtol=1e-5, atol=1e-6 * float(y.grad.abs().max() + 1e-30))
