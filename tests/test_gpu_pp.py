"""GPU tier of the off-centre principal point (gs_scene.Camera.cx / cy; GS_FRAME_PRINCIPAL_POINT, gs_seed_apply_pp and
gs_view_overlap_pp of include/gs_abi.h) through the frame path, the inference paths, the pose gradient, seeding and the overlap
count.  The yardstick is tests/pp_testutil.PPOracleFrame -- the oracle's own pipeline with the projected centre shifted -- and,
independently of every helper, the closed form of one Gaussian on the optical axis (test_on_axis_gaussian_lands_on_the_principal_
point).  Standards: the pair list bit for bit, the image test's abs 5e-5 (scaled by the depth range for the depth map), gradients
by gs_testutil.assert_grads_close with its defaults.  Tracking and the mapping loop: tests/test_gpu_pp_slam.py.

Shapes: 5,000 Gaussians at 128 x 96 (no padding), 120 x 90 (padded on both axes) and 121 x 91 (odd: the 0.5 of cx0); the offsets
of pp_testutil.OFFSETS.  The inference paths need the strip variant: 140,000 Gaussians at 320 x 240 and 300 x 232, the shapes of
tests/test_gpu_scene_pack.py::test_culled_static_pose."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import overlap_ref as R
import pp_testutil as P
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_geometry import principal_point_default, principal_point_offset
from gs_scene import Scene, make_camera
from gs_testutil import assert_grads_close, robust_aux_grads, to_torch
from seed_ref import select
from test_gpu_aux import check_maps
from test_gpu_frame import case

pytestmark = pytest.mark.gpu

IMG_ATOL = 5e-5
OFF_A, OFF_B, OFF_C = P.OFFSETS
_FRAMES = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frame(W, H, off, sh=0, method="prob2", dist=0.5, exp=False):
    """(scene, offset camera, PPOracleFrame, renderer keywords), computed once per process and shared: read only."""
    key = (W, H, off, sh, method, dist, exp)
    if key not in _FRAMES:
        scene, cam = case(5000, W, H, seed=7, use_sh=bool(sh), sh_degree=sh or 2)
        cam = P.offset_camera(cam, off)
        of_kw, r_kw = {}, {}
        if exp:
            scene.scale = np.log(np.abs(scene.scale) + 1e-4).astype(np.float32)
            of_kw["scale_activation"] = r_kw["scale_activation"] = "exp"
        if method != "prob2":
            of_kw.update(tile_culling_method=method, dist_thresh=dist)
            r_kw.update(tile_culling_method=method, tile_culling_dist_thresh=dist)
        _FRAMES[key] = (scene, cam, P.PPOracleFrame(scene, cam, **of_kw), r_kw)
    return _FRAMES[key]


# --------------------------------------------------------------------------------------- 5. the frame against the shifted oracle
CONFIGS = [
    ("120x90 +7.3 -4.6", dict(W=120, H=90, off=OFF_A)),
    ("120x90 +21.25 -18.5", dict(W=120, H=90, off=OFF_B)),
    ("120x90 -70.5 +3.0", dict(W=120, H=90, off=OFF_C)),
    ("128x96", dict(W=128, H=96, off=OFF_B)),
    ("121x91", dict(W=121, H=91, off=OFF_B)),
    ("sh2", dict(W=120, H=90, off=OFF_B, sh=2)),
    ("sh3", dict(W=120, H=90, off=OFF_B, sh=3)),
    ("prob", dict(W=120, H=90, off=OFF_B, method="prob")),
    ("dist", dict(W=120, H=90, off=OFF_B, method="dist")),
    ("exp", dict(W=120, H=90, off=OFF_B, exp=True)),
    ("bwd_rows", dict(W=120, H=90, off=OFF_B), dict(bwd_rows=True)),
    ("no bwd_rows", dict(W=120, H=90, off=OFF_B), dict(bwd_rows=False)),
    # the other project kernels: the table variant's fused project + count, and the plain project kernel of the radix modes
    ("table", dict(W=120, H=90, off=OFF_B), dict(table_bin=True)),
    ("radix", dict(W=120, H=90, off=OFF_B), dict(sort_mode=0)),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_frame_matches_the_shifted_oracle(gpu, cfg):
    """An inference frame with emitted keys: visible count, pair count, the (tile, depth bits, Gaussian) list, the stored
    centres and covariances bit for bit, the image within 5e-5.  A training aux frame: pair list, image, depth and alpha maps,
    and the five parameter gradients of <gimg, image> + <gd, depth> + <ga, alpha> element by element."""
    name, fkw, extra = cfg if len(cfg) == 3 else (*cfg, {})
    scene, cam, of, r_kw = _frame(**fkw)
    r_kw = dict(r_kw, **extra)
    assert principal_point_offset(cam) != (0.0, 0.0) and int(of.mask.sum()) > 500 and len(of.ids) > 2000, name
    params = to_torch(scene, gpu)
    grow = fkw.get("method") == "dist"  # (the rows of a "dist" frame cover the discs' bounding squares)
    cap = dict(max_pairs=max(len(of.ids), 64), auto_grow=True) if grow else dict(max_pairs=len(of.ids) + 17, auto_grow=False)
    r = FrameRenderer(gpu, training=False, emit_sorted_keys=True, **cap, **{k: v for k, v in r_kw.items() if k != "bwd_rows"})
    image, _ = r.forward(*params, cam)
    if grow:
        image, _ = r.forward(*params, cam)
    assert r._frame.flags & _lib.GS_FRAME_PRINCIPAL_POINT
    if "table_bin" in extra:
        assert r.binning_variant() == "table"
    elif "sort_mode" not in extra:
        assert r.binning_variant() == "strip"
    st = r.stats()
    assert (st.overflow, st.visible, st.pairs) == (0, int(of.mask.sum()), len(of.ids)), (name, st)
    v = r.debug_views()
    assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys), "sorted (tile, depth) keys differ"
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids), "sorted Gaussian ids differ"
    vis = of.mask.astype(bool)
    geom = v["rec_geom"].cpu().numpy()
    assert np.array_equal(geom[vis, :3].view(np.uint32), of.pos_i[vis].view(np.uint32)) and np.all(geom[~vis] == 0)
    if not fkw.get("exp"):  # (expf against np.exp: the activated scales differ in the last bit before anything else happens)
        assert np.array_equal(v["rec_cov"].cpu().numpy()[vis].view(np.uint32), of.cov.reshape(-1, 4)[vis].view(np.uint32))
    err = float(np.abs(image.cpu().numpy() - of.image).max())
    print(f"PP frame {name}: visible {st.visible} pairs {st.pairs} image err {err:.2e}")
    assert err < IMG_ATOL, (name, err)
    # ---- training aux frame and its backward
    gimg, gd, ga, n_masked = robust_aux_grads(of, 17)
    assert n_masked < 0.005 * cam.width * cam.height, (name, n_masked)
    ref, scale = of.aux_backward(gimg, gd, ga, with_scale=True)
    rt = FrameRenderer(gpu, training=True, **cap, **r_kw)
    out = rt.forward(*params, cam, aux=True)
    if grow:
        rt.auto_grow = False
        out = rt.forward(*params, cam, aux=True)
    timg, _, depth, alpha = out
    assert rt._frame.flags & _lib.GS_FRAME_PRINCIPAL_POINT and rt._frame.flags & _lib.GS_FRAME_AUX
    if "bwd_rows" in extra:
        assert bool(rt._frame.flags & _lib.GS_FRAME_BWD_ROWS) == extra["bwd_rows"]
    assert rt.stats().pairs == len(of.ids)
    assert np.array_equal(rt.debug_views()["sorted_ids"].cpu().numpy(), of.ids)
    assert float(np.abs(timg.cpu().numpy() - of.image).max()) < IMG_ATOL
    check_maps(of, depth, alpha, rt._aux_keep[2])
    t = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    got = [x.cpu().numpy() for x in rt.backward(t(gimg), grad_depth=t(gd), grad_alpha=t(ga))]
    rep = assert_grads_close(got, ref, scale, f"principal point, {name}")
    print(f"PP grads {name}:", {k: (v[0], "%.2e" % v[2]) for k, v in rep.items()}, "(worst err/tol, rel. L2)")
    for x in got:
        assert np.all(x[~vis] == 0)


@pytest.mark.parametrize("aux", [False, True])
def test_fused_step_equals_backward_then_adam(gpu, aux):
    """backward_adam / backward_adam(aux) of an offset frame against backward + FusedAdam.step() on the same frames: parameters,
    both moments and the gradient statistic bit for bit (the unfused backward is the one held against the oracle above)."""
    from test_gpu_rgbd import _assert_same, _fused_pair

    scene, cam, of, _ = _frame(120, 90, OFF_B)
    got = _fused_pair(gpu, scene, cam, "max", True, 3, max_pairs=1 << 18, aux=aux)
    _assert_same(got, "max")
    centred = copy.copy(cam)
    centred.cx = centred.cy = None
    other = _fused_pair(gpu, scene, centred, "max", True, 3, max_pairs=1 << 18, aux=aux)
    assert not torch.equal(got[0][0], other[0][0])  # (the offset reached the fused step: another camera, another fit)


# ------------------------------------------------------------------------ 6. an anchor that does not pass through the helper
@pytest.mark.parametrize("W,H", P.SIZES)
@pytest.mark.parametrize("off", P.OFFSETS)
def test_on_axis_gaussian_lands_on_the_principal_point(gpu, W, H, off):
    """One isotropic Gaussian on the optical axis (identity pose, pos = (0, 0, z), sigma_px = fx s / z = 3): the alpha map is
    opa exp(-((i + 0.5 - cx)^2 + (j + 0.5 - cy)^2) / (2 sigma_px^2)) within 5e-5 on every pixel within 2 sigma_px of (cx, cy)
    -- the sign of the offset and the half-pixel convention, fixed without principal_point_offset or the oracle.  cx0, cy0 are
    written out here: W / 2 for an even size, (W + 1) / 2 for an odd one.  (-70.5 puts the principal point outside the image:
    no pixel lies within 2 sigma; the pixels on which the Gaussian still exceeds 0.06 -- inside the bounding box of its 0.05
    level set, which is what the tiles are listed from: a few at width 128, none at 120 and 121 -- are held to the same
    formula.)"""
    cx = (W / 2 if W % 2 == 0 else (W + 1) / 2) + off[0]
    cy = (H / 2 if H % 2 == 0 else (H + 1) / 2) + off[1]
    fx, z, sigma_px, opa_logit = 0.75 * W, 4.0, 3.0, 1.5
    s = sigma_px * z / fx
    scene = Scene(np.array([[0.0, 0.0, z]], np.float32), np.array([[1.0, 0.0, 0.0, 0.0]], np.float32),
                  np.full((1, 3), s - 1e-4, np.float32), np.array([opa_logit], np.float32), np.zeros((1, 3), np.float32))
    cam = make_camera(W, H)
    cam.cx, cam.cy = cx, cy
    r = FrameRenderer(gpu, max_pairs=4096, training=False, auto_grow=False)
    _, _, _, alpha = r.forward(*to_torch(scene, gpu), cam, aux=True)
    assert r.stats().visible == 1
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d2 = (ii + 0.5 - cx) ** 2 + (jj + 0.5 - cy) ** 2
    want = 1.0 / (1.0 + np.exp(-opa_logit)) * np.exp(-d2 / (2.0 * sigma_px ** 2))
    err = np.abs(alpha.cpu().numpy().astype(np.float64) - want)
    near = d2 <= (2.0 * sigma_px) ** 2
    level = np.exp(-d2 / (2.0 * sigma_px ** 2)) >= 0.06
    print(f"PP anchor {W}x{H} {off}: {int(near.sum())} pixels within 2 sigma, {int(level.sum())} above 0.06, "
          f"max err {float(err[level].max()) if level.any() else 0.0:.2e}")
    if off != OFF_C:
        assert int(near.sum()) >= 100  # (a disc of radius 6 pixels, all of it inside the image)
    else:
        assert not near.any()
        assert float(alpha.max()) <= float(want.max()) + IMG_ATOL  # (nothing brighter than the closed form allows)
    if (near | level).any():
        assert err[near | level].max() < IMG_ATOL


# ------------------------------------------------------------------------------------------------ 7. zero offset is absent
def test_a_spelled_out_centre_is_no_offset(gpu):
    """cx0, cy0 given explicitly: the frame is unflagged and image, records, gradients, seeds and overlap counts are those of
    the camera without them, bit for bit."""
    from gs_seed import seed_from_depth
    from gs_slam import KeyframeSet

    for W, H in ((120, 90), (121, 91)):
        scene, cam = case(5000, W, H, seed=7)
        spelled = P.offset_camera(cam, (0.0, 0.0))
        assert spelled.cx is not None and (spelled.cx, spelled.cy) == principal_point_default(W, H)
        params = to_torch(scene, gpu)
        g = torch.Generator(device=gpu).manual_seed(5)
        gimg, gd, ga = (torch.randn(s, generator=g, device=gpu) for s in ((H, W, 3), (H, W), (H, W)))
        outs = []
        for c in (cam, spelled):
            r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=False, emit_sorted_keys=True)
            img, pad, d, a = r.forward(*params, c, aux=True)
            assert not (r._frame.flags & _lib.GS_FRAME_PRINCIPAL_POINT)
            v = {k: t.clone() for k, t in r.debug_views().items()}
            grads = [x.clone() for x in r.backward(gimg, grad_depth=gd, grad_alpha=ga)]
            outs.append((img.clone(), pad.clone(), d.clone(), a.clone(), v, grads))
        a, b = outs
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(_bits(x), _bits(y))
        assert set(a[4]) == set(b[4])
        for k in a[4]:
            assert torch.equal(_bits(a[4][k]) if a[4][k].dtype == torch.float32 else a[4][k],
                               _bits(b[4][k]) if b[4][k].dtype == torch.float32 else b[4][k]), k
        for x, y in zip(a[5], b[5]):
            assert torch.equal(_bits(x), _bits(y))
        # seeds and overlap counts
        z = torch.from_numpy(R.range_map(H, W, seed=3)).to(gpu)
        image = torch.rand(H, W, 3, generator=g, device=gpu)
        s0, s1 = seed_from_depth(image, z, cam, stride=2), seed_from_depth(image, z, spelled, stride=2)
        assert s0[0].shape[0] > 100 and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(s0, s1))
        counts = []
        for c in (cam, spelled):
            ks = KeyframeSet(4, gpu)
            ks.add(c, image, z)
            moved = copy.copy(c)
            moved.tran = np.asarray(c.tran, np.float32) + np.array([0.3, 0.0, 0.1], np.float32)
            ks.add(moved, image, z)
            counts.append(ks.overlap(z, c, stride=2, border=0))
        assert np.array_equal(counts[0], counts[1]) and 0 < counts[0][1] < counts[0][0] == counts[0][2]


# ------------------------------------------------------------------------------------------------------ 8. inference paths
@pytest.mark.parametrize("w,h", [(320, 240), (300, 232)])
def test_culled_and_packed_frames_of_an_offset_camera(gpu, w, h):
    """tests/test_gpu_scene_pack.py::test_culled_static_pose with an offset camera: frames 2 - 5 are occlusion-culled and read
    the scene pack, do not fall back, drop pairs, and equal a fresh raw renderer's first frame bit for bit.  Then the dilated
    and the near variant of the cull (a pose 2 pixels and 0.1 pixel away), two cameras that differ only in cx alternated on one
    renderer, and culling_mask() of a culled frame against the shifted oracle's mask."""
    from test_gpu_scene_pack import MAX_PAIRS, N, _fresh_raw, _opaque, _opaque_arrays, _same_frame

    params = _opaque(gpu, N, w, h)
    cam = P.offset_camera(make_camera(w, h), OFF_A)
    kw = dict(max_pairs=MAX_PAIRS, auto_grow=False)
    r = FrameRenderer(gpu, **kw)
    off = FrameRenderer(gpu, scene_pack=False, occlusion_cull=False, **kw)
    ref, _ = off.forward(*params, cam)
    full_pairs = off.stats().pairs
    centred_ref = _fresh_raw(gpu, params, make_camera(w, h))
    assert not _same_frame(ref, centred_ref)
    for k in range(5):
        r._cull_off_until = 0  # (the adaptive policy kept out of the way)
        img, _ = r.forward(*params, cam)
        st = r.stats()
        assert r._frame.flags & _lib.GS_FRAME_PRINCIPAL_POINT
        assert _same_frame(img, ref), k
        assert bool(r._frame.flags & _lib.GS_FRAME_OCCLUSION_CULL) == (k >= 1) and r.scene_pack_active() == (k >= 1), k
        assert not st.cull_fallback and st.overflow == 0, (k, st)
        if k >= 1:
            assert st.pairs < 0.6 * full_pairs, (k, st.pairs, full_pairs)
    # culling_mask() of the culled frame: the reference-API operator knows no offset
    scene = _opaque_arrays(N, w, h, 21, False)
    _, _, want = P.shifted_projection(scene, cam)
    got = r.culling_mask().cpu().numpy()
    assert np.array_equal(got, want.astype(bool)) and 0 < int(want.sum()) < N
    centred_mask = P.shifted_projection(scene, make_camera(w, h))[2].astype(bool)
    assert (centred_mask != want.astype(bool)).sum() > 100  # (the offset moves the frustum: the masks differ)
    # the dilated (2 pixels) and the near (0.1 pixel) variant, armed by a small yaw from the recorded pose
    f = float(cam.focal_x)
    for shift_px, flags in ((2.0, _lib.GS_FRAME_CULL_DILATE), (0.1, _lib.GS_FRAME_CULL_DILATE | _lib.GS_FRAME_CULL_DILATE_NEAR)):
        r._cull_off_until = 0
        r.forward(*params, cam)  # (records the cuts of `cam` again)
        near_cam = P.offset_camera(make_camera(w, h, yaw_deg=float(np.degrees(shift_px / f))), OFF_A)
        r._cull_off_until = 0
        img, _ = r.forward(*params, near_cam)
        fl = int(r._frame.flags)
        assert fl & _lib.GS_FRAME_OCCLUSION_CULL and (fl & (_lib.GS_FRAME_CULL_DILATE | _lib.GS_FRAME_CULL_DILATE_NEAR)) == flags
        assert fl & _lib.GS_FRAME_PRINCIPAL_POINT and r.stats().overflow == 0
        assert _same_frame(img, _fresh_raw(gpu, params, near_cam)), shift_px
    # two cameras that differ only in cx, alternated: neither is served the other's descriptor, constants or cuts
    other = copy.copy(cam)
    other.cx = cam.cx + 3.0
    refs = {id(cam): ref, id(other): _fresh_raw(gpu, params, other)}
    assert not _same_frame(refs[id(cam)], refs[id(other)])
    for k in range(6):
        c = (cam, other)[k % 2]
        r._cull_off_until = 0
        img, _ = r.forward(*params, c)
        assert _same_frame(img, refs[id(c)]), k
        if k >= 1:  # (another principal point than the frame before: its cuts do not carry over)
            assert not (r._frame.flags & _lib.GS_FRAME_OCCLUSION_CULL), k


# ---------------------------------------------------------------------------------------------------------- 9. pose gradient
@pytest.mark.parametrize("aux", [False, True])
def test_pose_gradient_of_an_offset_camera(gpu, aux):
    from test_gpu_pose import _identity_case, check_pose_gradient

    scene, cam = case(5000, 128, 96, seed=31)
    cam = P.offset_camera(cam, OFF_B)
    worst = check_pose_gradient(gpu, scene, cam, aux, of=P.PPOracleFrame(scene, cam))
    print(f"PP pose gradient aux={aux}: worst err/tol {worst:.3f}")
    scene, cam = case(5000, 128, 96, seed=41)
    r = _identity_case(gpu, scene, P.offset_camera(cam, OFF_B), aux, False, 43)
    assert r._frame.flags & _lib.GS_FRAME_PRINCIPAL_POINT


def test_render_with_a_pose_keeps_the_offset(gpu):
    scene, cam = case(5000, 128, 96, seed=73)
    cam = P.offset_camera(cam, OFF_A)
    params = to_torch(scene, gpu)
    base = P.offset_camera(make_camera(128, 96), OFF_A)  # identity pose: the pose tensors carry case()'s
    rot, tran = torch.from_numpy(cam.rot.copy()), torch.from_numpy(cam.tran.copy())
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    a = r.render(*params, cam)
    assert torch.equal(a, r.render(*params, base, pose=(rot, tran)))
    centred = copy.copy(cam)
    centred.cx = centred.cy = None
    assert not torch.equal(a, r.render(*params, centred))
    ai, ad, aa = r.render_aux(*params, cam)
    bi, bd, ba = r.render_aux(*params, base, pose=(rot.to(gpu), tran.to(gpu)))
    assert torch.equal(ai, bi) and torch.equal(ad, bd) and torch.equal(aa, ba)


# ------------------------------------------------------------------------------------------------------------- 10. seeding
def _seed_camera(W, H, off):
    cam = make_camera(W, H, yaw_deg=17.0)
    cam.focal_y = 0.8 * W  # fx != fy
    cam.tran = np.array([0.4, -0.3, 0.8], np.float32)
    return P.offset_camera(cam, off)


@pytest.mark.parametrize("off", [OFF_A, OFF_C], ids=["+7.3 -4.6", "-70.5 +3.0"])
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("stride", [1, 3])
def test_seeds_of_an_offset_camera(gpu, stride, with_maps, off):
    """A 40 x 30 frame: the selected pixels are seed_ref.select's (the decision sees no camera); position and scale rows equal
    the float32 restatement of the moved ray bit for bit, for rgb and degree-2 SH rows alike; the rows that do not depend on
    the camera (quaternion, opacity, colour: logf is not restated) equal the centred camera's bit for bit; and every seeded
    position, projected in fp64 with u = fx x / z + cx, lands within 1e-3 pixel of its pixel's centre."""
    from gs_seed import seed_from_depth
    from test_gpu_seed import _inputs

    H, W = 30, 40
    cam = _seed_camera(W, H, off)
    D, A, z, img = _inputs(H, W, seed=H + W + stride)
    at, fr, sf, p0 = 0.5, 0.1, 0.7, 0.9
    sel, meas = select(z, D if with_maps else None, A if with_maps else None, stride, at, fr)
    ys, xs = np.nonzero(sel)
    assert 10 < len(ys) and (not with_maps or len(ys) < int(meas.sum()))
    tD, tA, tz, timg = (torch.from_numpy(x).to(gpu) for x in (D, A, z, img))
    kw = dict(rendered=(tD, tA) if with_maps else None, stride=stride, alpha_thresh=at, front_rel=fr, scale_factor=sf,
              opa_init=p0)
    want_pos, want_scale = P.seed_rows_f32(z, cam, ys, xs, stride, sf)
    centred = copy.copy(cam)
    centred.cx = centred.cy = None
    for cd in (3, 27):
        pos, quat, scale, opa, rgb = (t.cpu().numpy() for t in seed_from_depth(timg, tz, cam, color_dim=cd, **kw))
        assert pos.shape == (len(ys), 3) and rgb.shape == (len(ys), cd)
        assert np.array_equal(pos.view(np.uint32), want_pos.view(np.uint32))
        for k in range(3):
            assert np.array_equal(scale[:, k].view(np.uint32), want_scale.view(np.uint32))
        plain = [t.cpu().numpy() for t in seed_from_depth(timg, tz, centred, color_dim=cd, **kw)]
        assert not np.array_equal(plain[0], pos)
        for got, ref in ((quat, plain[1]), (opa, plain[3]), (rgb, plain[4])):
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        p_c = pos.astype(np.float64) @ np.asarray(cam.rot, np.float64).T + np.asarray(cam.tran, np.float64)
        px = float(np.float32(cam.focal_x)) * p_c[:, 0] / p_c[:, 2] + cam.cx
        py = float(np.float32(cam.focal_y)) * p_c[:, 1] / p_c[:, 2] + cam.cy
        err = max(np.abs(px - (xs + 0.5)).max(), np.abs(py - (ys + 0.5)).max())
        print(f"PP seed stride {stride} maps={with_maps} {off} cd={cd}: {len(ys)} seeds, reprojection error {err:.2e} px")
        assert err < 1e-3


# ------------------------------------------------------------------------------------------------------------- 11. overlap
def _overlap_views(k):
    """The views of overlap_ref.case given assorted offsets: the frame's own camera with the frame's offset (every point falls
    back on its pixel), the same pose with an offset that ALONE moves every point out of its image, the rest cycling through
    offsets that include none at all."""
    W = k["cam"].width
    cycle = [(0.0, 0.0), OFF_A, (-2.25, 6.5), (0.5, -0.5), (11.0, 3.75)]
    views = []
    for i, v in enumerate(k["views"]):
        if i == 0:
            views.append(P.offset_camera(v, OFF_A))
        elif i == 3:
            views.append(P.offset_camera(k["views"][0], (OFF_A[0] + 2.0 * W, OFF_A[1])))
        else:
            views.append(P.offset_camera(v, cycle[i % len(cycle)]) if cycle[i % len(cycle)] != (0.0, 0.0) else v)
    return views


@pytest.mark.parametrize("Hc,Wc,stride,n_views", [(37, 53, 1, 65), (64, 64, 3, 6), (120, 160, 2, 7)])
def test_overlap_counts_with_offsets(gpu, Hc, Wc, stride, n_views):
    from gs_slam import KeyframeSet, view_overlap

    k = R.case(Hc, Wc, stride, n_views)
    cam = P.offset_camera(k["cam"], OFF_A)
    views = _overlap_views(k)
    z = torch.from_numpy(k["z"]).to(gpu)
    ks = KeyframeSet(max(n_views, 1), gpu)
    for v in views:
        ks.add(v, None, None)
    assert ks.table_pp[:n_views].cpu().numpy().tobytes() == \
        np.array([principal_point_offset(v) for v in views], np.float32).tobytes()
    for border in (0, 4):
        got = ks.overlap(z, cam, stride=stride, near=k["near"], border=border)
        want = P.overlap_counts_f32(k["z"], cam, views, stride, k["near"], border)
        assert np.array_equal(got, want), (border, got, want)
        assert got[0] == R.own_view_count(k["z"], stride, border)  # its own camera and offset
        assert got[3] == 0 and 0 < got[n_views]                    # the offset alone: nothing of the frame is seen
    # the frame has an offset, no view has: still the *_pp kernel (the frame's rays moved)
    plain = KeyframeSet(max(n_views, 1), gpu)
    for v in k["views"]:
        plain.add(v, None, None)
    got = plain.overlap(z, cam, stride=stride, near=k["near"], border=0)
    assert np.array_equal(got, P.overlap_counts_f32(k["z"], cam, k["views"], stride, k["near"], 0))
    # no offset anywhere: what gs_view_overlap returns (the call IS gs_view_overlap), through every door
    want = R.counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], 0)
    assert np.array_equal(plain.overlap(z, k["cam"], stride=stride, near=k["near"], border=0), want)
    zeros = torch.zeros_like(plain.table_pp)
    assert np.array_equal(view_overlap(z, k["cam"], plain.table, n_views, stride, k["near"], 0, zeros).cpu().numpy(), want)
    from gs_seed import seed_camera_pp

    cpp = seed_camera_pp(k["cam"])
    opts = _lib.GsOverlapOpts(stride, k["near"], 0)
    ws = torch.empty(int(_lib.gs_view_overlap_workspace_bytes(Hc, Wc, stride, n_views)), dtype=torch.uint8, device=gpu)
    counts = torch.full((n_views + 2,), -1, dtype=torch.int64, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(_lib.gs_view_overlap_pp(z.data_ptr(), C.byref(cpp), plain.table.data_ptr(), None, n_views, C.byref(opts),
                                           counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream(gpu).cuda_stream), "gs_view_overlap_pp")
    assert np.array_equal(counts.cpu().numpy(), want)
