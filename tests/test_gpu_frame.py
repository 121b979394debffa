"""GPU parity of the fused frame path (gs_frame_forward / gs_frame_backward) against the
oracle's restatement of Splatter.forward + autograd (tests/gs_testutil.OracleFrame).

 * sorted (tile, depth_bits, gaussian_id) list and tile ranges: BIT-EXACT;
 * projected records: bit-exact (same fp32 expression order on both sides);
 * image: abs 5e-5;
 * parameter gradients: ELEMENT-WISE |got - ref| <= 1e-4 |ref| + 1e-5 scale, `scale` being the element's own
   conditioning scale (the sum of the magnitudes of the terms it is made of, computed by the oracle next to the
   gradient: gs_testutil.grad_close), plus a relative L2 bound per tensor -- on small scenes and at the BASELINE
   sizes (cfg2, cfg3, cfg4 with SH).  dL/dimage is zero on the few pixels (~0.1 %) whose transmittance passes
   within 1e-4 (relative) of the 1e-4 stop threshold: there one Gaussian more or less is a legitimate fp32 outcome
   and the two sides would not be adding up the same terms (OracleFrame.robust_grad_image).  The gradient path has no atomics: the sums run in a fixed order and the
   result is bitwise repeatable; what differs from the oracle is that order, v_exp_f32 / v_rcp_f32, and the
   conic hoisted out of the pixel loop.
"""
import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import OracleFrame, assert_error_no_worse_than, assert_grads_close, to_torch

pytestmark = pytest.mark.gpu

IMG_ATOL = 5e-5


def case(n, W, H, seed=7, use_sh=False, yaw=2.0, sh_degree=2):
    scene = make_scene(n, W, H, seed=seed, use_sh=use_sh, sh_degree=sh_degree)
    cam = make_camera(W, H, yaw_deg=yaw)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    return scene, cam


def mode_kwargs(sort_mode):
    """0, 1, 2 (= the default strip variant of sort_mode 2), "2t" (table variant), "2s" (slice-sorted variant)"""
    if sort_mode == "2s":
        return dict(sort_mode=2, slice_sort=True)
    if sort_mode == "2t":
        return dict(sort_mode=2, table_bin=True)
    return dict(sort_mode=sort_mode)


def check_forward(gpu, scene, cam, training=False, sort_mode=2, emit_sorted_keys=False, img_atol=IMG_ATOL,
                  long_lists=None, of=None, r_kw=None):
    # (``of``: the caller's frame of this scene and camera, shared; ``r_kw``: further FrameRenderer options, passed through)
    of = OracleFrame(scene, cam) if of is None else of
    if long_lists is None:  # scenes with lists beyond the LDS window exercise the long-list kernels
        long_lists = bool(np.diff(of.accum).max() > 2048)
    r = FrameRenderer(gpu, max_pairs=max(len(of.ids) + 17, 64), training=training, auto_grow=False,
                      emit_sorted_keys=emit_sorted_keys, long_lists=long_lists, **mode_kwargs(sort_mode), **(r_kw or {}))
    params = to_torch(scene, gpu)
    image, padded = r.forward(*params, cam)
    st = r.stats()
    assert st.overflow == 0
    assert st.visible == int(of.mask.sum())
    assert st.pairs == len(of.ids)
    v = r.debug_views()
    keys = v["sorted_keys"].cpu().numpy().view(np.uint64)
    ids = v["sorted_ids"].cpu().numpy()
    assert np.array_equal(keys, of.keys), "sorted (tile, depth) keys differ from the oracle"
    assert np.array_equal(ids, of.ids), "sorted Gaussian ids differ from the oracle"
    ranges = v["tile_ranges"].cpu().numpy()
    nonempty = of.accum[1:] > of.accum[:-1]
    assert np.array_equal(ranges[nonempty, 0], of.accum[:-1][nonempty])
    assert np.array_equal(ranges[nonempty, 1], of.accum[1:][nonempty])
    assert np.all(ranges[~nonempty] == 0)
    vis = of.mask.astype(bool)
    geom = v["rec_geom"].cpu().numpy()
    assert np.array_equal(geom[vis, :3].view(np.uint32), of.pos_i[vis].view(np.uint32))
    assert np.all(geom[~vis] == 0)
    assert np.array_equal(v["rec_cov"].cpu().numpy()[vis].view(np.uint32), of.cov.reshape(-1, 4)[vis].view(np.uint32))
    err = np.abs(image.cpu().numpy() - of.image).max()
    assert err < img_atol, err
    if padded is not None:
        assert np.abs(padded.cpu().numpy() - of.padded).max() < IMG_ATOL
    return of, r, params


@pytest.mark.parametrize("sort_mode", [2, "2t"])
@pytest.mark.parametrize("n,W,H", [(10_000, 256, 256), (30_000, 333, 201), (2_000, 64, 48), (3_000, 40, 200)])
def test_frame_forward_parity(gpu, n, W, H, sort_mode):
    # 2: the strip variant (default); "2t": the table variant (GS_FRAME_TABLE_BIN, what small scenes take).
    # 333 x 201 and 40 x 200: tile rows that end inside a strip / inside its first half
    check_forward(gpu, *case(n, W, H), sort_mode=sort_mode)


@pytest.mark.parametrize("sort_mode", [0, 1, "2s"])
def test_frame_forward_parity_fallback_variants(gpu, sort_mode):
    """Round 6: the round-1 variants are no longer part of the frame path's test matrix -- sort_mode 0 / 1 (LSD radix on
    the 64-bit key / on the tile bits; mode 1 is what grids beyond the LDS counters fall back to,
    test_frame_forward_more_tiles_than_lds_counters) and the slice-sorted binning ("2s") are checked once here and at
    full size in test_full_size_sortedness_and_mode_equivalence; gs_sort_pairs has its own test (test_gpu_kernels.py)."""
    check_forward(gpu, *case(30_000, 333, 201), sort_mode=sort_mode)


@pytest.mark.parametrize("sort_mode", [2, "2t"])
def test_frame_forward_giant_bucket_sorted_in_chunks(gpu, sort_mode):
    # > 4096 pairs in one tile: the per-tile sort handles 2048-key chunks in LDS and the strides >= 2048 of the
    # last merge levels through global memory (the packed, the (key, id) and the gathered input variants)
    scene, cam = case(40_000, 32, 32, seed=8)
    of, _, _ = check_forward(gpu, scene, cam, sort_mode=sort_mode)
    assert np.diff(of.accum).max() > 4096


def test_long_list_kernels_follow_the_longest_list_statistic(gpu):
    """A frame with one 7,000-Gaussian pile: the first frame walks the pile with one wave; its counters report the longest list
    (gs_frame_longest_list_async, read back with the stats), and the renderer sets GS_FRAME_LONG_LISTS from then on.
    Images of the two paths agree; long_lists=False never switches."""
    scene, cam = case(10_000, 256, 256, seed=37)
    pile = np.arange(3000, 10_000)
    rng = np.random.default_rng(2)
    scene.pos[pile] = scene.pos[0] + rng.normal(scale=0.002, size=(len(pile), 3)).astype(np.float32)
    scene.scale[pile] = np.float32(0.003)
    scene.opa[pile] = -7.0
    of = OracleFrame(scene, cam)
    assert np.diff(of.accum).max() > 4096 and len(of.ids) / 256 < 1024
    params = to_torch(scene, gpu)
    auto = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=True)
    never = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=True, long_lists=False)
    first, _ = auto.forward(*params, cam)
    assert auto.stats().longest_list == int(np.diff(of.accum).max()) and auto._long_lists_seen
    second, _ = auto.forward(*params, cam)
    assert auto._frame.flags & 16  # GS_FRAME_LONG_LISTS
    ref, _ = never.forward(*params, cam)
    ref2, _ = never.forward(*params, cam)
    assert not (never._frame.flags & 16)
    assert torch.equal(first, ref) and torch.equal(ref, ref2)
    assert float((second - ref).abs().max()) < 1e-5
    assert np.abs(second.cpu().numpy() - of.image).max() < 1e-3
    v = auto.debug_views()
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)


def test_lists_beyond_the_sort_window_switch_the_sort_alone(gpu):
    """Round 6: 768 tiles with lists of 2,200 - 2,900 pairs each (beyond the per-tile sort's 2,048-pair LDS window; the device
    is busy with them, so cutting them into segments would only add work): the renderer sets GS_FRAME_LONG_SORT (128) from
    the second frame on and NOT GS_FRAME_LONG_LISTS (16) -- the lists go to big_list_sort_kernel, the compositing keeps
    its one-wave walk (the cost model of FrameRenderer._note_lists).  The sort is exact in every variant, so the flagged
    frame's list AND image equal the first frame's bit for bit.  Six tiles with lists of 4,100 - 5,000 and nothing else on
    the device, on the other hand, DO take the segments: the same model."""
    scene, cam = make_scene(240_000, 512, 384, seed=8, max_px_sigma=40.0), make_camera(512, 384)
    scene.opa -= 4.0
    of = OracleFrame(scene, cam)
    lens = np.diff(of.accum)
    assert (lens > 2048).sum() > 500 and lens.max() < 4096
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=True, emit_sorted_keys=True)
    first, _ = r.forward(*params, cam)
    assert not (r._frame.flags & (16 | 128))
    assert r.stats().longest_list == int(lens.max()) and r._long_sort_seen and not r._long_lists_seen
    ids_first = r.debug_views()["sorted_ids"].clone()
    second, _ = r.forward(*params, cam)
    assert (r._frame.flags & 128) and not (r._frame.flags & 16) and r.binning_variant() == "strip"
    v = r.debug_views()
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids) and torch.equal(v["sorted_ids"], ids_first)
    assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys)
    assert torch.equal(first, second)
    assert np.abs(second.cpu().numpy() - of.image).max() < IMG_ATOL
    # training frames too: same image, gradients bit-identical with and without the flag (the backward never looks at it)
    g = torch.randn(384, 512, 3, device=gpu)
    grads = []
    for flagged in (False, True):
        rt = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False)
        rt._long_sort_seen = flagged
        img, _ = rt.forward(*params, cam)
        assert bool(rt._frame.flags & 128) == flagged and torch.equal(img, first)
        grads.append([t.clone() for t in rt.backward(g)])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    # six long lists on an otherwise idle device: the model asks for the segments
    few, cam2 = make_scene(14_000, 48, 32, seed=8), make_camera(48, 32)
    r2 = FrameRenderer(gpu, max_pairs=1 << 16, auto_grow=True)
    a, _ = r2.forward(*to_torch(few, gpu), cam2)
    st = r2.stats()
    assert 4096 < st.longest_list <= 6144 and r2._long_sort_seen
    # (make_scene's opacities stop these tiles' pixels after a few hundred Gaussians: the longest WALK is short, no segments;
    # the same lists with faint Gaussians are walked to their end -- 5,000 steps of one wave on an idle device: segments)
    assert not r2._long_lists_seen
    few.opa[:] = -7.0
    r3 = FrameRenderer(gpu, max_pairs=1 << 16, auto_grow=True)
    a, _ = r3.forward(*to_torch(few, gpu), cam2)
    assert r3.stats().longest_list == st.longest_list and r3._long_lists_seen
    b, _ = r3.forward(*to_torch(few, gpu), cam2)
    assert (r3._frame.flags & 16) and float((a - b).abs().max()) < 1e-5


# ------------------------------------------------------------------ temporal occlusion cull (GS_FRAME_OCCLUSION_CULL)
def _dense_case(n=60_000, W=192, H=128, seed=3, yaw=0.0):
    scene = make_scene(n, W, H, seed=seed)
    scene.opa += 3.0  # opaque: every tile's pixels stop long before the end of its list
    return scene, make_camera(W, H, yaw_deg=yaw)


def test_occlusion_cull_static_camera_is_bit_exact(gpu):
    """Round 6.  The second and later inference frames of a renderer drop, at emission, the pairs behind the depth at which
    the previous frame saw all pixels of their tile stop: fewer pairs emitted and sorted, no fallback, and the image is
    BIT-identical to the first (unculled) frame's and to a renderer with the cull off; it matches the oracle."""
    scene, cam = _dense_case()
    of = OracleFrame(scene, cam)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=False, occlusion_cull=False)
    first, _ = r.forward(*params, cam)
    st1 = r.stats()
    assert not (r._frame.flags & 256) and st1.pairs == len(of.ids) and not st1.cull_fallback
    assert np.abs(first.cpu().numpy() - of.image).max() < IMG_ATOL
    for _ in range(3):
        img, _ = r.forward(*params, cam)
        st = r.stats()
        assert r._frame.flags & 256 and r.binning_variant() == "strip"
        assert st.pairs < 0.6 * len(of.ids) and st.visible == st1.visible and st.overflow == 0 and not st.cull_fallback
        assert torch.equal(img, first)
        ref, _ = off.forward(*params, cam)
        assert not (off._frame.flags & 256) and off.stats().pairs == len(of.ids) and torch.equal(ref, first)
    # frames that must keep their full lists: training, exported sorted keys
    rt = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=False, training=True)
    rk = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=False, emit_sorted_keys=True)
    for rr in (rt, rk):
        for _ in range(2):
            rr.forward(*params, cam)
            assert rr.stats().pairs == len(of.ids)
    assert np.array_equal(rk.debug_views()["sorted_ids"].cpu().numpy(), of.ids)


def test_occlusion_cull_moving_camera_falls_back_and_stays_exact(gpu):
    """A camera that creeps, jumps and comes back; then another scene (thin: nothing saturates) and another Gaussian count in
    the same workspace.  Every frame equals, bit for bit, the frame of a renderer with the cull off -- under three policies:
      identical pose only (CULL_MAX_SHIFT_PX = 0): only exact repeats of a pose are culled, with the tiles' own cuts;
      the default (8 px): poses near the recorded one are culled with GS_FRAME_CULL_DILATE (every tile's cut from its 3 x 3
        neighbourhood, pushed back in depth), jumps are left alone;
      lifted (inf, the adaptive switch kept out of the way): every frame but the first is culled; after a jump a tile runs
        past its cut and the library renders the frame again from the full lists.
    Whether the trimmed lists sufficed or the second pass ran, the image is exact; both happen.  Spot checks against the
    oracle."""
    scene, _ = _dense_case()
    params = to_torch(scene, gpu)
    off = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False, occlusion_cull=False)
    # a viewer's path: rests, small steps (a fraction of a degree, millimetres), a few jumps
    yaws = [0.0, 0.0, 0.0, 0.002, 0.002, 0.1, 0.15, 0.2, 0.3, 4.0, 4.0, 30.0, 30.0, -20.0, 0.0, 0.0]
    DILATE = 512
    for policy in ("identical", "default", "lifted"):
        r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
        if policy != "default":
            r.CULL_MAX_SHIFT_PX = float("inf") if policy == "lifted" else 0.0
        fell, clean, not_culled, dilated, dilated_clean, culled_share = 0, 0, 0, 0, 0, []
        for k, yaw in enumerate(yaws):
            cam = make_camera(192, 128, yaw_deg=yaw)
            cam.tran = np.array([0.002 * (k // 2), -0.001 * (k // 2), 0.0], np.float32)
            if policy == "lifted":
                r._cull_off_until = 0  # (and the adaptive policy kept out of the way: a fallback would switch the cull off)
            img, _ = r.forward(*params, cam)
            st = r.stats()
            ref, _ = off.forward(*params, cam)
            full = off.stats().pairs
            assert torch.equal(img, ref), (policy, k, yaw, st)
            if not (r._frame.flags & 256):
                not_culled += 1
                assert st.pairs == full and not st.cull_fallback and not (r._frame.flags & DILATE)
                continue
            fell += int(st.cull_fallback)
            clean += int(not st.cull_fallback)
            dilated += int(bool(r._frame.flags & DILATE))
            dilated_clean += int(bool(r._frame.flags & DILATE) and not st.cull_fallback)
            if not st.cull_fallback:
                culled_share.append(1.0 - st.pairs / full)
            else:
                assert st.pairs == full  # the counters are those of the second, untrimmed pass
            if k in (1, 10, 15):
                assert np.abs(img.cpu().numpy() - OracleFrame(scene, cam).image).max() < IMG_ATOL
        print("occlusion cull over the camera path, policy", policy, "| fell back", fell, "clean", clean, "not culled",
              not_culled, "dilated", dilated, "of which clean", dilated_clean, "culled share", [round(c, 2) for c in culled_share])
        if policy == "lifted":
            assert not_culled == 1 and fell >= 2 and clean >= 3 and dilated >= 8, (fell, clean, not_culled, dilated)
        elif policy == "identical":
            # culled: the exact repeats of a pose (k = 1 and k = 15: they cannot run past their cuts); every frame whose
            # pose differs from the previous one's, by however little, is left alone
            assert fell == 0 and clean == 2 and not_culled == 14 and dilated == 0, (fell, clean, not_culled, dilated)
        else:
            # the jumps (k = 9, 11, 13, 14: 9 pixels and more at this focal length) are never culled; the creeping frames are,
            # with dilated cuts, unless a fallback has switched the cull off on the way
            assert not_culled >= 5 and dilated >= 1 and dilated_clean >= 1, (fell, clean, not_culled, dilated, dilated_clean)
        assert max(culled_share) > 0.4, culled_share
    cam = make_camera(192, 128, yaw_deg=1.0)
    # another scene in the same workspace: thin (no tile saturates -> the cut table it leaves is all GS_NO_CUT) ...
    thin = make_scene(20_000, 192, 128, seed=9)
    thin.opa[:] = -4.0
    p_thin = to_torch(thin, gpu)
    for k in range(3):
        img, _ = r.forward(*p_thin, cam)
        st = r.stats()
        ref, _ = off.forward(*p_thin, cam)
        assert torch.equal(img, ref) and (k == 0 or not st.cull_fallback)
        assert k == 0 or st.pairs == off.stats().pairs  # nothing to cull
    # ... and back to the dense one with another Gaussian count (the table's place in the workspace does not depend on N)
    dense2, _ = _dense_case(n=45_000, seed=11)
    p2 = to_torch(dense2, gpu)
    r._cull_off_until, r._cull_backoff = 0, 256  # (the adaptive policy has switched the cull off by now: next test)
    for k in range(3):
        img, _ = r.forward(*p2, cam)
        ref, _ = off.forward(*p2, cam)
        assert torch.equal(img, ref)
    assert r.stats().pairs < off.stats().pairs and not r.stats().cull_fallback


@pytest.mark.parametrize("qcap,stash,method,act", [(None, None, "prob2", "abs"), (2048, 256, "prob2", "abs"),
                                                   (512, 0, "prob2", "abs"), (None, None, "prob", "abs"),
                                                   (None, None, "prob2", "exp")])
def test_occlusion_cull_compacting_project_paths(gpu, monkeypatch, qcap, stash, method, act):
    """The compacting project kernel of a culled frame at a size where a slice takes several rounds (1.2 M Gaussians: 4,864
    per slice) -- and, with the chunk and stash capacities shrunk through the environment, several CHUNKS per slice (a slice
    has more than 16,384 Gaussians only beyond 4.2 M) and survivors beyond the LDS stash (their positions gathered from
    memory again).  Static pose (the tiles' own cuts), a creeping pose (dilated cuts), a jump with the policy lifted
    (fallback): every image bit-identical to the unculled renderer's.  "prob" listing: no Gaussian-level test, lists
    trimmed all the same."""
    if qcap is not None:
        monkeypatch.setenv("GS_OCC_QCAP", str(qcap))
        monkeypatch.setenv("GS_OCC_STASH", str(stash))
    W, H, n = 640, 384, 1_200_000
    scene = make_scene(n, W, H, seed=5)
    scene.opa += 3.0
    if act == "exp":  # (the occlusion test bounds the footprint by the largest ACTIVATED scale: exp through v_exp_f32)
        scene.scale[:] = np.log(scene.scale)
    params = to_torch(scene, gpu)
    kw = dict(max_pairs=6_000_000, auto_grow=False, tile_culling_method=method, scale_activation=act)
    r, off = FrameRenderer(gpu, **kw), FrameRenderer(gpu, occlusion_cull=False, **kw)
    r.CULL_MAX_SHIFT_PX = float("inf")
    yaws = [0.0, 0.0, 0.0, 0.01, 0.02, 0.03, 25.0, 25.0, 25.01]
    culled = fell = dilated = 0
    emitted = []
    for k, yaw in enumerate(yaws):
        cam = make_camera(W, H, yaw_deg=yaw)
        r._cull_off_until = 0
        img, _ = r.forward(*params, cam)
        st = r.stats()
        ref, _ = off.forward(*params, cam)
        assert torch.equal(img, ref), (k, yaw, st)
        full = off.stats().pairs
        assert full <= 6_000_000 and st.overflow == 0
        culled += int(bool(r._frame.flags & 256))
        dilated += int(bool(r._frame.flags & 512))
        fell += int(st.cull_fallback)
        if (r._frame.flags & 256) and not st.cull_fallback:
            emitted.append(st.pairs / full)
    print("compacting project paths:", qcap, stash, method, act, "| culled", culled, "dilated", dilated, "fell back", fell,
          "emitted share", [round(e, 3) for e in emitted])
    assert culled == len(yaws) - 1 and dilated >= 4 and min(emitted) < 0.6, (culled, dilated, fell, emitted)


@pytest.mark.parametrize("deg", [2, 3])
def test_occlusion_cull_sh_frames_are_bit_exact(gpu, deg):
    """SH colours (inference): the same front end, the SH compositing kernel writes the cut table.  Static and creeping pose,
    bit-identical to the unculled renderer's images; against the oracle at degree 2."""
    W, H = 192, 128
    scene = make_scene(60_000, W, H, seed=3, use_sh=True, sh_degree=deg)
    scene.opa += 3.0
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False, occlusion_cull=False)
    culled = 0
    for k, yaw in enumerate([0.0, 0.0, 0.0, 0.01, 0.02]):
        cam = make_camera(W, H, yaw_deg=yaw)
        img, _ = r.forward(*params, cam)
        st = r.stats()
        ref, _ = off.forward(*params, cam)
        assert torch.equal(img, ref), (k, st)
        if r._frame.flags & 256:
            culled += 1
            assert st.pairs < 0.6 * off.stats().pairs and not st.cull_fallback
        if deg == 2 and k == 2:
            assert np.abs(img.cpu().numpy() - OracleFrame(scene, cam).image).max() < IMG_ATOL
    assert culled >= 2


def test_occlusion_cull_with_degenerate_gaussians(gpu):
    """Gaussians nobody should train towards -- NaN / infinite positions, zero, huge, NaN and infinite scales, a zero quaternion,
    infinite opacities -- mixed into the dense scene: the occlusion test leaves everything it cannot bound to the exact
    arithmetic (a NaN scale slips through fmaxf, a huge one fails the 16-tile limit, a NaN position fails every comparison), so
    the culled frames equal the unculled renderer's bit for bit, NaN pixels included."""
    scene, cam = _dense_case()
    rng = np.random.default_rng(9)
    k = 40
    idx = rng.choice(len(scene.pos), size=8 * k, replace=False).reshape(8, k)
    scene.pos[idx[0]] = np.nan
    scene.pos[idx[1], 2] = np.inf
    scene.scale[idx[2]] = 0.0
    scene.scale[idx[3]] = 1e30
    scene.scale[idx[4], 1] = np.nan
    scene.scale[idx[5], 0] = np.inf
    scene.quat[idx[6]] = 0.0
    scene.opa[idx[7][: k // 2]] = np.inf
    scene.opa[idx[7][k // 2:]] = -np.inf
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False, occlusion_cull=False)
    r.CULL_MAX_SHIFT_PX = float("inf")
    culled = 0
    for yaw in (0.0, 0.0, 0.0, 0.02, 0.05, 3.0, 3.0):
        c = make_camera(192, 128, yaw_deg=yaw)
        r._cull_off_until = 0
        img, _ = r.forward(*params, c)
        st = r.stats()
        ref, _ = off.forward(*params, c)
        assert st.overflow == 0 and off.stats().overflow == 0
        assert torch.equal(torch.isnan(img), torch.isnan(ref)), (yaw, st)
        assert torch.equal(torch.nan_to_num(img), torch.nan_to_num(ref)), (yaw, st)
        culled += int(bool(r._frame.flags & 256))
    assert culled == 6


@pytest.mark.parametrize("seed", [1, 2])
def test_occlusion_cull_random_walk_is_bit_exact(gpu, seed):
    """tools/cull_fuzz.py in small: 160 frames of a random camera walk (rests, yaw steps between 0.001 and 3 degrees, small
    translations) under the renderer's own policy -- own cuts at rest, dilated cuts near the recorded pose, none beyond,
    adaptive back-off -- against a renderer with the cull off, bit for bit."""
    scene, _ = _dense_case(n=150_000, W=320, H=208, seed=17)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False, occlusion_cull=False)
    rng = np.random.default_rng(seed)
    yaw = tx = 0.0
    culled = dilated = 0
    for k in range(160):
        u = rng.random()
        if 0.25 <= u < 0.9:
            yaw = float(np.clip(yaw + np.exp(rng.uniform(np.log(0.001), np.log(3.0))) * (1 if rng.random() < 0.5 else -1), -20, 20))
        elif u >= 0.9:
            tx += float(rng.normal(0.0, 0.003))
        cam = make_camera(320, 208, yaw_deg=yaw)
        cam.tran = np.asarray(cam.tran, np.float32) + np.array([tx, 0.0, 0.0], np.float32)
        img, _ = r.forward(*params, cam)
        ref, _ = off.forward(*params, cam)
        assert torch.equal(img, ref), (k, yaw, int(r._frame.flags), r.stats())
        culled += int(bool(r._frame.flags & 256))
        dilated += int(bool(r._frame.flags & 512))
    assert culled >= 20 and dilated >= 5, (culled, dilated)


def test_culling_mask_of_an_occlusion_culled_frame(gpu):
    """A culled frame writes the records of its projected Gaussians only: ``culling_mask()`` of such a frame re-runs the
    frustum test (the reference's global_culling operator) and equals the mask of the unculled frame; ``debug_views()``
    refuses."""
    scene, cam = _dense_case()
    params = to_torch(scene, gpu)
    off = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False, occlusion_cull=False)
    off.forward(*params, cam)
    want = off.culling_mask()
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
    for k in range(3):
        r.forward(*params, cam)
        assert torch.equal(r.culling_mask(), want), k
    assert r._frame.flags & 256 and r.stats().pairs < off.stats().pairs
    with pytest.raises(RuntimeError):
        r.debug_views()


def test_occlusion_cull_switches_itself_off_where_it_does_not_pay(gpu):
    """A scene whose tiles do not saturate (nothing to cull): the renderer looks at the counters of its first unculled and
    first culled frame (asynchronous, tagged copies), finds that the cull dropped less than a third of the pairs, and
    switches it off for 256 frames -- those frames carry no flag, i.e. none of the gated launches.  On the opaque scene
    it stays on.  Images identical throughout."""
    thin = make_scene(30_000, 192, 128, seed=9)
    thin.opa[:] = -4.0
    cam = make_camera(192, 128)
    for scene, stays_on in ((thin, False), (_dense_case()[0], True)):
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=False)
        first, _ = r.forward(*params, cam)
        flags = []
        for k in range(12):
            img, _ = r.forward(*params, cam)
            flags.append(bool(r._frame.flags & 256))
            assert torch.equal(img, first)
            torch.cuda.synchronize()  # (lets the probes land: a free-running loop decides a few frames later)
        assert flags[0], flags  # the frame right behind the first one is culled: nothing is known yet
        if stays_on:
            assert all(flags) and r._cull_settled and r._cull_off_until == 0, flags
        else:
            assert not any(flags[4:]) and r._cull_off_until > r._frame_serial and not r._cull_settled, flags


def test_small_scene_with_a_pile_switches_to_the_long_list_kernels(gpu):
    """below 131,072 Gaussians sort_mode 2 takes the TABLE variant, whose kernels used to report 0 for the
    longest list -- a small scene with a pile-up (the case the long-list kernels were built for) stayed on the serial path
    for ever.  Now the table variant reports its longest list too, the renderer latches GS_FRAME_LONG_LISTS, and a frame
    with that flag takes the strip variant (which owns the long-list kernels) whatever the scene size."""
    scene, cam = case(10_000, 256, 256, seed=37)
    pile = np.arange(3000, 10_000)
    rng = np.random.default_rng(2)
    scene.pos[pile] = scene.pos[0] + rng.normal(scale=0.002, size=(len(pile), 3)).astype(np.float32)
    scene.scale[pile] = np.float32(0.003)
    scene.opa[pile] = -7.0
    of = OracleFrame(scene, cam)
    longest = int(np.diff(of.accum).max())
    assert longest > 4096
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=True, force_strips=False)  # the library's own choice
    first, _ = r.forward(*params, cam)
    assert r.binning_variant() == "table" and not (r._frame.flags & 16)
    st = r.stats()
    assert st.longest_list == longest and r._long_lists_seen, (st, r._stats_host.tolist(), int(r._frame.flags))
    second, _ = r.forward(*params, cam)
    assert r._frame.flags & 16 and r.binning_variant() == "strip"  # GS_FRAME_LONG_LISTS => strips + long-list kernels
    assert float((second - first).abs().max()) < 1e-5
    assert np.array_equal(r.debug_views()["sorted_ids"].cpu().numpy(), of.ids)
    # an explicit long_lists=True on a small scene no longer falls through to the table variant either
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, auto_grow=False, force_strips=False, long_lists=True)
    third, _ = r2.forward(*params, cam)
    assert r2.binning_variant() == "strip" and torch.equal(third, second)


@pytest.mark.parametrize("kw", [dict(force_strips=False), dict(force_strips=True), dict(sort_mode=0), dict(sort_mode=1)],
                         ids=["table", "strip", "radix64", "radix_tile_bits"])
def test_counters_do_not_depend_on_what_the_workspace_held_before(gpu, kw):
    """Round 6: the compositing kernel adds its walk statistics onto counters that only the strip variant reset -- in the
    table variant a workspace fresh from the allocator kept whatever was there (a value with the top bit set reads as a
    negative walk: a small scene with a pile-up never got its long-list flag; a positive one flags a harmless scene).  Here
    the workspace is handed over filled with 0xFF: every counter the host acts upon is the frame's own."""
    scene, cam = case(10_000, 256, 256, seed=37)
    params = to_torch(scene, gpu)
    ref = FrameRenderer(gpu, max_pairs=1 << 20, auto_grow=False, **kw)
    ref.forward(*params, cam)
    want = ref.stats()
    r = FrameRenderer(gpu, max_pairs=1 << 20, auto_grow=False, **kw)
    r._ws = torch.full((ref._ws.numel() + (1 << 20),), 0xFF, dtype=torch.uint8, device=gpu)
    img, _ = r.forward(*params, cam)
    st = r.stats()
    h = r._stats_host.tolist()
    assert (st.visible, st.pairs, st.overflow, st.longest_list) == (want.visible, want.pairs, 0, want.longest_list)
    # [9] longest list, [10] ran past a cut, [12] pairs beyond 512 per tile, [13] longest walk, [14] steps beyond 512
    assert h[9] == want.longest_list and h[10] == 0 and h[12] == 0 and h[13] == 0 and h[14] == 0, h
    assert not r._long_lists_seen and not r._long_sort_seen and not st.cull_fallback
    assert torch.equal(img, ref.forward(*params, cam)[0])


@pytest.mark.parametrize("use_sh", [False, True])
@pytest.mark.parametrize("strips", [False, True], ids=["table", "strip"])
def test_training_frame_does_not_depend_on_what_the_workspace_held_before(gpu, strips, use_sh):
    """The backward reads only what the forward and its own kernels wrote (gradient rows are never zero-filled: unwritten
    ones must never be read; checkpoints, work lists, stop keys likewise): a forward + backward in a workspace handed over
    filled with 0xFF gives the image and all five gradients of a clean renderer, bit for bit."""
    W, H = 192, 128
    scene = make_scene(20_000, W, H, seed=21, use_sh=use_sh)
    cam = make_camera(W, H, yaw_deg=2.0)
    params = to_torch(scene, gpu)
    g = torch.Generator(device=gpu).manual_seed(4)
    grad = torch.randn(H, W, 3, device=gpu, generator=g) / (H * W)
    kw = dict(max_pairs=1 << 20, auto_grow=False, training=True, force_strips=strips)
    ref = FrameRenderer(gpu, **kw)
    img0, _ = ref.forward(*params, cam)
    g0 = [t.clone() for t in ref.backward(grad)]
    r = FrameRenderer(gpu, **kw)
    r._ws = torch.full((ref._ws.numel() + (1 << 20),), 0xFF, dtype=torch.uint8, device=gpu)
    img1, _ = r.forward(*params, cam)
    g1 = r.backward(grad)
    assert r.binning_variant() == ("strip" if strips else "table")
    assert torch.equal(img0, img1)
    for a, b, name in zip(g0, g1, ("pos", "quat", "scale", "opa", "rgb")):
        assert torch.equal(a, b), name
    st0, st1 = ref.stats(), r.stats()
    assert (st0.visible, st0.pairs, st0.buckets, st0.saturated_buckets) == (st1.visible, st1.pairs, st1.buckets, st1.saturated_buckets)


@pytest.mark.parametrize("use_sh", [False, True])
def test_long_lists_composited_in_segments(gpu, use_sh):
    """Dense frame with low-opacity pile-ups: every tile's pixels are still alive after 4096 Gaussians, so the rest
    of each list (up to ~12,000 here; beyond the first GS_LONG_MIN = 512 since round 5) is composited in segments of
    GS_SEG_LEN = 512 by separate waves (transmittance products ->
    incoming transmittance -> per-segment colours -> combine; raster_fwd_segment.hip).  Against the one-wave-per-tile walk of
    the same build (GS_FRAME_SERIAL_LONG_LISTS): image, processed counts and all five parameter gradients must agree to
    the rounding of the transmittance that enters a segment; against the oracle: the list exactly, the image to 1e-3
    (a chain of 10,000 layers is conditioned like that in fp32 whoever walks it)."""
    scene, cam = case(50_000, 64, 64, seed=31, use_sh=use_sh)
    scene.opa[:] = -6.0
    of = OracleFrame(scene, cam)
    assert np.diff(of.accum).min() > 4096 and np.diff(of.accum).max() > 4096 + 2 * 2048
    outs = []
    for serial in (False, True):
        params = to_torch(scene, gpu, requires_grad=True)
        r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False, serial_long_lists=serial,
                          long_lists=True)
        img = r.render(*params, cam)
        assert r.stats().pairs == len(of.ids)
        steps = r.composited_steps()
        g = torch.from_numpy(np.random.default_rng(3).normal(size=of.image.shape).astype(np.float32)).to(gpu)
        img.backward(g)
        outs.append((img.detach().cpu().numpy(), steps, [t.grad.cpu().numpy() for t in params]))
    (img_a, steps_a, grads_a), (img_b, steps_b, grads_b) = outs
    assert np.abs(img_a - of.image).max() < 1e-3
    assert np.abs(img_a - img_b).max() < 1e-5  # partial colours are added in a different association
    assert steps_a == steps_b  # the same processed range, by either walk (nothing stops early here)
    for ga, gb, name in zip(grads_a, grads_b, ("pos", "quat", "scale", "opa", "rgb")):
        assert np.isfinite(ga).all()
        assert np.abs(ga - gb).max() <= 2e-4 * np.abs(gb).max() + 1e-30, name


# tolerance of the seam test below: gs_testutil's standard element-wise criterion (kappa x 1, relative L2 2e-5) -- measured
# on the first run (profiles/r05_a_full_size_gradient_parity.txt): worst element at 0.12 x its tolerance with kappa x 4,
# relative L2 1.3e-6 ... 9.6e-6 per tensor -- the 5,000-layer chains are what the oracle's conditioning scale is for
LONG_KAPPA_X = 1.0
LONG_L2 = 2e-5


@pytest.mark.parametrize("sh_degree", [2, 3])
def test_long_lists_sh_backward_hand_over_matches_oracle(gpu, sh_degree):
    """the SH backward of frames flagged GS_FRAME_LONG_LISTS was only compared with the serial walk
    of the same build, never with the oracle.  Round 4 had the matrix-pipe kernel take a tile's first 32 buckets and hand the
    rest to raster_backward_pixel_sh_kernel (one wave per bucket); since round 5 the matrix-pipe kernel takes work items of at
    most 8 buckets, several workgroups per long tile, and there is no hand-over (raster_bwd_mfma.hip: mfma_items_kernel) -- either
    way it is this test that puts the long-list backward against the oracle: every tile's list is 60 - 96 buckets deep (3,900 -
    6,150 Gaussians of opacity 0.0067: pixels stop at T <= 1e-4 around the 4,600th layer, i.e. deep inside the list, in
    another work item than the one that started the tile; the forward composites the lists in segments) and all five gradients
    meet the oracle's draw_backward + index sum + projection backward (gaussian.cu:440-803, splatter.py:604-613,
    gaussian.cu:1371-1576) element by element."""
    scene, cam = case(30_000, 64, 64, seed=33, use_sh=True, sh_degree=sh_degree)
    scene.opa[:] = -5.0
    of = OracleFrame(scene, cam)
    lens = np.diff(of.accum)
    assert lens.min() > 32 * 64 + 4 * 64 and lens.max() > 4096, (lens.min(), lens.max())  # every tile: several work items
    gimg = np.random.default_rng(12).normal(size=of.image.shape).astype(np.float32)
    gimg, n_masked = of.robust_grad_image(gimg)
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False, long_lists=True)
    img = r.render(*params, cam)
    assert r._frame.flags & 16  # GS_FRAME_LONG_LISTS
    assert r.stats().pairs == len(of.ids)
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < 1e-3
    img.backward(torch.from_numpy(gimg).to(gpu))
    report = assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, f"long-list seam, degree {sh_degree}",
                                kappa=LONG_KAPPA_X * 3e-5, l2=LONG_L2)
    print(f"long-list seam, degree {sh_degree}: lists {lens.min()} .. {lens.max()}, masked pixels {n_masked};", report)


@pytest.mark.parametrize("sort_mode", [2, "2t"])
@pytest.mark.parametrize("n,W,H", [(10_000, 256, 256), (40_000, 32, 32)])
def test_frame_forward_emitted_sorted_keys(gpu, n, W, H, sort_mode):
    """GS_FRAME_EMIT_SORTED_KEYS: the per-tile sort also writes the sorted (tile << 32 | depth bits) keys (the default
    frame only writes the ids; debug_views() then rebuilds the keys from the records).  In the strip variant the key
    buffer doubles as the scratch of lists beyond the LDS window (40,000 Gaussians on four tiles: the dense-frame
    queue + big_list_sort_kernel), so the written keys are checked on both paths."""
    check_forward(gpu, *case(n, W, H, seed=8), sort_mode=sort_mode, emit_sorted_keys=True)


def test_frame_forward_dense_frame_with_depth_clusters(gpu):
    """GS_FRAME_LONG_LISTS: lists beyond the LDS window are queued for big_list_sort_kernel.  40,000 Gaussians on four tiles, on 10 sites of 4,000 exact copies each: every depth bin of a
    list holds thousands of equal keys -- more than the window -- and takes the chunked bitonic sort inside that kernel;
    300 sites: bins of ~130 copies go through the distribution sort's large-bucket path."""
    for n_sites in (10, 300):
        scene, cam = case(40_000, 32, 32, seed=29)
        site = np.arange(scene.n) % n_sites
        scene.pos[:] = scene.pos[site]
        scene.scale[:] = scene.scale[site]
        scene.quat[:] = scene.quat[site]
        scene.opa[:] = -9.0
        # 10,000 coincident layers per pixel: the image's own fp32 conditioning (a transmittance chain of 10,000 steps)
        # is not what this test is about -- the (tile, depth, id) list is compared exactly, the image to 1e-3
        of, _, _ = check_forward(gpu, scene, cam, sort_mode=2, img_atol=1e-3)
        assert np.diff(of.accum).max() > 4096


@pytest.mark.parametrize("n_sites,jitter", [(40, 0.0), (300, 0.0), (40, 1e-6), (3000, 0.0)])
def test_frame_forward_depth_clusters(gpu, n_sites, jitter):
    """The strip variant sorts a tile's list by ONE counting pass over buckets that are linear in the depth bits and
    only ranks inside a bucket; depth clusters (Gaussians on one surface) put many keys into one bucket, which is then
    sorted by the bitonic network (a wave up to 512 keys, the workgroup beyond).  30,000 Gaussians on 40 / 300 / 3000
    sites: 750 / 100 / 10 exact copies per site (equal depth bits: the order inside a cluster is by Gaussian index),
    and 40 sites with a relative jitter of 1e-6 (distinct depths a few ulp apart).  The list must be the oracle's."""
    scene, cam = case(30_000, 256, 256, seed=23)
    site = np.arange(scene.n) % n_sites
    rng = np.random.default_rng(5)
    scene.pos[:] = scene.pos[site] * (1.0 + jitter * rng.standard_normal((scene.n, 1))).astype(np.float32)
    scene.scale[:] = scene.scale[site]
    scene.quat[:] = scene.quat[site]
    scene.opa[:] = -3.0  # nearly transparent: every pixel stays live through the long lists
    of, _, _ = check_forward(gpu, scene, cam, sort_mode=2)
    assert np.diff(of.accum).max() > 500  # 3000 sites: lists of up to ~520 (one wave each); 40 sites: thousands


@pytest.mark.parametrize("sort_mode,n_big", [(2, 230)])
def test_frame_forward_slice_larger_than_the_lds_staging_buffer(gpu, sort_mode, n_big):
    """The strip variant's scatter stages the ENTRIES of a slice (one per strip of eight
    tiles a Gaussian crosses: 125 per screen-filling Gaussian here, 230 of them = ~29 k against ~19.9 k slots) and
    stores the ones that do not fit straight to their final place; the half strips then hold far more than the 4096
    pairs of the LDS sort window and take the global path."""
    scene, cam = case(2_000, 640, 400, seed=41)
    big = np.arange(n_big)
    scene.scale[big] = np.float32(3.0) * np.abs(scene.pos[big, 2:3]) / cam.focal_x * 200 * np.array([1.0, 0.7, 0.85], np.float32)
    scene.pos[big, :2] *= 0.05
    scene.pos[big, 2] = np.linspace(3.0, 8.0, len(big), dtype=np.float32)
    scene.opa[big] = -4.0
    of, r, _ = check_forward(gpu, scene, cam, sort_mode=sort_mode)
    counts = np.bincount(of.ids, minlength=scene.n)
    assert counts[big].sum() > 40_000  # far more than the ~19 k pairs the staging buffer holds at this tile count


@pytest.mark.parametrize("sort_mode", [2, "2t"])
def test_frame_forward_more_tiles_than_lds_counters(gpu, sort_mode):
    """4096 x 2176 = 34,816 tiles: above the 32,768 LDS counters of the table variant of sort_mode 2, which must fall
    back to the tile-bit radix passes (mode 1) and still produce the oracle's list and image; the strip variant needs
    one counter per strip (4,352 here) and handles the frame itself."""
    scene, cam = case(4_000, 4096, 2176, seed=17)
    of, r, _ = check_forward(gpu, scene, cam, sort_mode=sort_mode)
    assert r.stats().pairs == len(of.ids) > 0


def test_frame_forward_4k_uses_lds_counters(gpu):
    """3840 x 2160 = 32,400 tiles: just inside the 32,768 LDS counters (127 KiB of dynamic LDS per workgroup)."""
    scene, cam = case(6_000, 3840, 2160, seed=19)
    of, r, _ = check_forward(gpu, scene, cam, sort_mode=2)
    assert r.stats().pairs == len(of.ids) > 0


def test_frame_tile_culling_method_prob(gpu):
    """--tile_culling_method prob (gaussian.cu:138-195: bounding box against the tiles' edges) on the fused path:
    the pair list equals the oracle's calc_tile_list method 1 (itself bit-identical to the reference kernel), the
    frame and its gradients follow.  (The list differs from prob2's only for bounding boxes that touch a tile edge
    exactly; what is checked is that THIS code path reproduces the reference's edge comparisons.)"""
    scene, cam = case(15_000, 250, 186, seed=29)
    of = OracleFrame(scene, cam, tile_culling_method="prob")
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 7, training=True, auto_grow=False, tile_culling_method="prob")
    img = r.render(*params, cam)
    v = r.debug_views()
    assert r.stats().pairs == len(of.ids)
    assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys)
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < IMG_ATOL
    gimg = np.random.default_rng(6).normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
    img.backward(torch.from_numpy(gimg).to(gpu))
    ref, scale = of.backward(gimg, with_scale=True)
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, "prob")


@pytest.mark.parametrize("dist_thresh,W,H", [(0.5, 250, 186), (0.3, 333, 201), (1.0, 96, 80)])
def test_frame_tile_culling_method_dist(gpu, dist_thresh, W, H):
    """--tile_culling_method dist (gaussian.cu:101-136; Splatter.__init__'s own default): every tile whose CENTRE is
    closer than tile_length_x / dist_thresh to the Gaussian's centre, whatever its size -- a disc of tiles, not a
    rectangle.  The fused path walks the disc's bounding square with the reference's per-tile fp32 test: the pair
    list equals the oracle's calc_tile_list method 0 (itself bit-identical to the reference kernel) bit for bit,
    image and gradients follow (the gradient rows are laid out over the square, unlisted tiles hold zeros)."""
    scene, cam = case(12_000, W, H, seed=29)
    of = OracleFrame(scene, cam, tile_culling_method="dist", dist_thresh=dist_thresh)
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids), training=True, auto_grow=True, tile_culling_method="dist",
                      tile_culling_dist_thresh=dist_thresh)
    r.forward(*params, cam)  # grows the workspace to the sum of the bounding squares
    assert len(of.ids) < r.max_pairs < 12 * len(of.ids) + 8192
    r.auto_grow = False
    img = r.render(*params, cam)
    v = r.debug_views()
    st = r.stats()
    assert st.overflow == 0 and st.pairs == len(of.ids) > 0
    assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys)
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < IMG_ATOL
    gimg = np.random.default_rng(6).normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
    img.backward(torch.from_numpy(gimg).to(gpu))
    ref, scale = of.backward(gimg, with_scale=True)
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, "dist")
    # the rows of a "dist" frame cover the bounding squares: a capacity that holds the pairs but not the squares is
    # reported as overflow instead of silently dropping gradient rows
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) + 16, training=True, auto_grow=False, tile_culling_method="dist",
                       tile_culling_dist_thresh=dist_thresh)
    r2.forward(*to_torch(scene, gpu), cam)
    assert r2.stats().overflow > len(of.ids)
    with pytest.raises(ValueError):
        FrameRenderer(gpu, tile_culling_method="nearest")


@pytest.mark.parametrize("dist_thresh,n", [(0.5, 6_000), (0.2, 2_000)])
def test_frame_tile_culling_method_dist_sh_backward(gpu, dist_thresh, n):
    """"dist" listing with SH colours, backward: since round 5 the SH readers decide which gradient rows exist from the tiles'
    stop keys (a flag byte per row until then) -- and in a "dist" frame the rows are laid out over the disc's bounding SQUARE,
    of which only the listed tiles hold a row: the stop-key test alone would read the holes.  dist_thresh 0.5: discs of ~12
    tiles (the projection backward's own row walk); 0.2: ~80 tiles per Gaussian, beyond the 64 rows from which
    sh_big_rows_kernel sums a Gaussian's rows.  Gradients against the oracle, element by element."""
    scene, cam = case(n, 250, 186, seed=29, use_sh=True)
    scene.opa += 1.0  # some tiles saturate: rows behind the stop keys do not exist
    of = OracleFrame(scene, cam, tile_culling_method="dist", dist_thresh=dist_thresh)
    counts = np.bincount(of.ids, minlength=scene.n)
    assert (counts.max() > 64) == (dist_thresh < 0.3), counts.max()
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids), training=True, auto_grow=True, tile_culling_method="dist",
                      tile_culling_dist_thresh=dist_thresh)
    r.forward(*params, cam)  # grows the workspace to the sum of the bounding squares
    r.auto_grow = False
    img = r.render(*params, cam)
    assert r.stats().pairs == len(of.ids)
    assert np.array_equal(r.debug_views()["sorted_ids"].cpu().numpy(), of.ids)
    gimg = np.random.default_rng(6).normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)
    img.backward(torch.from_numpy(gimg).to(gpu))
    ref, scale = of.backward(gimg, with_scale=True)
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, f"dist, SH, thresh {dist_thresh}")


@pytest.mark.parametrize("sh_degree", [2, 3])
def test_frame_forward_sh(gpu, sh_degree):
    # degree 2 = the reference's 27 coefficients; degree 3 (48) is the extension BASELINE config 4 names
    check_forward(gpu, *case(8_000, 160, 96, use_sh=True, sh_degree=sh_degree))


def test_frame_sh_degree3_with_zero_band3_is_degree2(gpu):
    """Size-independent property: 48 coefficients with a zero degree-3 band render the degree-2 scene.  (Bit-exact
    in the oracle, tests/test_oracle_kat.py; the two kernel instantiations are compiled separately and the
    compiler's mul+add contraction differs in a few places, so here: to the last ulp or two.)"""
    import copy

    s3, cam = case(30_000, 320, 208, seed=21, use_sh=True, sh_degree=3)
    c = s3.rgb.reshape(-1, 3, 16)
    c[:, :, 9:] = 0
    s2 = copy.deepcopy(s3)
    s2.rgb = np.ascontiguousarray(c[:, :, :9]).reshape(-1, 27)
    gimg = torch.from_numpy(np.random.default_rng(3).normal(size=(208, 320, 3)).astype(np.float32)).to(gpu)
    outs = []
    for sc in (s3, s2):
        params = to_torch(sc, gpu, requires_grad=True)
        r = FrameRenderer(gpu, max_pairs=400_000, training=True)
        img = r.render(*params, cam)
        img.backward(gimg)
        outs.append((img.detach().clone(), [t.grad.clone() for t in params]))
    (i3, g3), (i2, g2) = outs
    assert float((i3 - i2).abs().max()) <= 2.5e-7
    for a, b in zip(g3[:4], g2[:4]):
        assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())
    b3 = g3[4].view(-1, 3, 16)
    assert float((b3[:, :, :9] - g2[4].view(-1, 3, 9)).abs().max()) <= 2e-6 * float(g2[4].abs().max())
    assert float(b3[:, :, 9:].abs().max()) > 0  # the zero band still receives its gradient


@pytest.mark.parametrize("sort_mode", [2])
def test_frame_forward_dense_tiles_multi_chunk(gpu, sort_mode):
    # ~1.5k Gaussians per tile: several 256-Gaussian LDS chunks per tile + early termination
    scene, cam = case(60_000, 96, 64, seed=3)
    scene.opa += 2.0
    of, _, _ = check_forward(gpu, scene, cam, sort_mode=sort_mode)
    assert np.diff(of.accum).max() > 500  # 3000 sites: lists of up to ~520 (one wave each); 40 sites: thousands


@pytest.mark.parametrize("use_sh", [False, True, 3])
def test_frame_backward_parity(gpu, use_sh):
    # use_sh: False = rgb logits, True = the reference's degree-2 SH, 3 = the degree-3 extension
    scene, cam = case(9_000 if use_sh else 20_000, 160, 112, seed=11, use_sh=bool(use_sh),
                      sh_degree=3 if use_sh == 3 else 2)
    of, r, _ = check_forward(gpu, scene, cam, training=True)
    rng = np.random.default_rng(4)
    gimg = rng.normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) + 5, training=True, auto_grow=False)
    img = r2.render(*params, cam)
    img.backward(torch.from_numpy(gimg).to(gpu))
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, f"sh={use_sh}")
    # culled Gaussians get exactly zero
    culled = of.mask == 0
    assert float(np.abs(params[0].grad.cpu().numpy()[culled]).max()) == 0.0


@pytest.mark.parametrize("sh_degree", [2, 3])
def test_frame_backward_sh_deep_saturating_tiles(gpu, sh_degree):
    """The SH backward on the matrix pipe (raster_bwd_mfma.hip: raster_backward_mfma_sh_kernel) where its structure shows: tiles
    several 64-Gaussian buckets deep (checkpoints, four waves sharing a tile), ragged last buckets and groups of 16,
    opaque Gaussians so that pixels -- and whole pixel rows, which the kernel then leaves out -- stop inside the list."""
    scene, cam = case(14_000, 96, 64, seed=5, use_sh=True, sh_degree=sh_degree)
    scene.opa += 1.5
    of, r, _ = check_forward(gpu, scene, cam, training=True)
    assert np.diff(of.accum).max() > 300  # several buckets per tile
    rng = np.random.default_rng(8)
    gimg = rng.normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) + 5, training=True, auto_grow=False)
    img = r2.render(*params, cam)
    img.backward(torch.from_numpy(gimg).to(gpu))
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, f"deep tiles, degree {sh_degree}")


def test_frame_backward_screen_filling_gaussians(gpu):
    """Gaussians that touch more than 256 tiles have their per-pair gradient rows summed by the whole workgroup
    (project_bwd.hip, deterministic tree) instead of by one thread: parity with the oracle for a scene that mixes a
    few of them -- next to each other in the array and isolated -- with ordinary ones, no SH and SH."""
    for use_sh in (False, True):
        scene, cam = case(3_000, 352, 272, seed=31, use_sh=use_sh)
        big = [10, 11, 12, 700, 2999]
        scene.scale[big] = np.float32(3.0) * np.abs(scene.pos[big, 2:3]) / cam.focal_x * 40 * \
            np.array([1.0, 0.55, 0.8], np.float32)  # anisotropic: an isotropic Gaussian has no quaternion gradient
        scene.pos[big, :2] *= 0.05
        scene.pos[big, 2] = np.linspace(3.0, 8.0, len(big), dtype=np.float32)
        scene.opa[big] = -2.0
        # ... and a few of 65 - 256 rows: beyond the rgb kernel's threshold for the workgroup's cooperative sum (64 rows since
        # round 4), below the SH pre-pass's (256), adjacent in the array as clones of a densification step are
        mid = [1500, 1501, 1503, 2200]
        scene.scale[mid] = np.float32(3.0) * np.abs(scene.pos[mid, 2:3]) / cam.focal_x * 13 * \
            np.array([1.0, 0.7, 0.85], np.float32)
        scene.pos[mid, :2] *= 0.3
        scene.pos[mid, 2] = np.linspace(4.0, 6.0, len(mid), dtype=np.float32)
        scene.opa[mid] = -2.5
        of = OracleFrame(scene, cam)
        counts = np.bincount(of.ids, minlength=scene.n)
        assert (counts[big] > 256).all() and counts.max() <= 22 * 17
        assert (counts[mid] > 64).all() and (counts[mid] <= 256).all(), counts[mid]
        big = big + mid
        gimg = np.random.default_rng(7).normal(size=of.image.shape).astype(np.float32)
        gimg, _ = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
        ref, scale = of.backward(gimg, with_scale=True)
        params = to_torch(scene, gpu, requires_grad=True)
        r = FrameRenderer(gpu, max_pairs=len(of.ids) + 9, training=True, auto_grow=False)
        img = r.render(*params, cam)
        assert np.abs(img.detach().cpu().numpy() - of.image).max() < IMG_ATOL
        img.backward(torch.from_numpy(gimg).to(gpu))
        grads = [t.grad.cpu().numpy() for t in params]
        assert_grads_close(grads, ref, scale, f"screen-filling sh={use_sh}")
        assert_grads_close([g[big] for g in grads], {k: v[big] for k, v in ref.items()},
                           {k: v[big] for k, v in scale.items()}, f"screen-filling sh={use_sh}, the big ones", l2=1e-4)


def test_frame_backward_exp_scale_activation(gpu):
    scene, cam = case(5_000, 96, 80, seed=13)
    scene.scale = np.log(np.abs(scene.scale) + 1e-4).astype(np.float32)
    of = OracleFrame(scene, cam, scale_activation="exp")
    gimg = np.random.default_rng(5).normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 5, training=True, scale_activation="exp", auto_grow=False)
    img = r.render(*params, cam)
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < 2e-4  # expf differs by ulps before projection
    img.backward(torch.from_numpy(gimg).to(gpu))
    # the activated scales differ by an ulp or two of expf before anything else happens: looser than "abs"
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, "exp", rtol=1e-3, kappa=1e-4, l2=1e-3)


def test_frame_all_culled_and_empty(gpu):
    scene, cam = case(500, 64, 64)
    scene.pos[:, 2] = -5.0  # everything behind the camera (splatter.py:563-564 returns zeros)
    r = FrameRenderer(gpu, max_pairs=1024, auto_grow=False)
    img, _ = r.forward(*to_torch(scene, gpu), cam)
    assert float(img.abs().max()) == 0.0
    st = r.stats()
    assert st.visible == 0 and st.pairs == 0


def test_frame_capacity_overflow_grows(gpu):
    scene, cam = case(10_000, 128, 128)
    of = OracleFrame(scene, cam)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) // 3, auto_grow=True)
    img, _ = r.forward(*to_torch(scene, gpu), cam)
    assert r.max_pairs >= len(of.ids)
    assert np.abs(img.cpu().numpy() - of.image).max() < IMG_ATOL
    r2 = FrameRenderer(gpu, max_pairs=len(of.ids) // 3, auto_grow=False)
    r2.forward(*to_torch(scene, gpu), cam)
    assert r2.stats().overflow == len(of.ids)  # reported, never silently dropped


@pytest.mark.parametrize("sort_mode", [2])
def test_frame_repeatable_bitwise(gpu, sort_mode):
    scene, cam = case(10_000, 128, 128)
    r = FrameRenderer(gpu, max_pairs=1 << 17, auto_grow=False, sort_mode=sort_mode)
    p = to_torch(scene, gpu)
    a = r.forward(*p, cam)[0].clone()
    b = r.forward(*p, cam)[0].clone()
    assert torch.equal(a, b)  # forward is deterministic (no atomics on the data path)


@pytest.mark.parametrize("bwd_rows", [False, True])
def test_frame_backward_repeatable_bitwise(gpu, bwd_rows):
    """No atomics anywhere on the gradient path: two backward passes give identical bits (both rgb kernels: the
    pixel-parallel one and the row-layout one of GS_FRAME_BWD_ROWS)."""
    scene, cam = case(15_000, 160, 112, seed=21)
    gimg = torch.from_numpy(np.random.default_rng(6).normal(size=(112, 160, 3)).astype(np.float32)).to(gpu)
    grads = []
    for _ in range(2):
        params = to_torch(scene, gpu, requires_grad=True)
        r = FrameRenderer(gpu, max_pairs=1 << 17, training=True, auto_grow=False, bwd_rows=bwd_rows)
        r.render(*params, cam).backward(gimg)
        assert bool(r._frame.flags & 64) == bwd_rows  # GS_FRAME_BWD_ROWS
        grads.append([t.grad.clone() for t in params])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def _rows_scenes():
    """(name, scene, camera) the row-layout rgb backward is checked on: deep tiles whose pixels stop inside the list (dead
    pixel rows are left out, several buckets per tile, ragged groups of 16), Gaussian counts around the group / bucket
    sizes, a nearly transparent scene (nothing stops: no row is ever left out), and screen-filling Gaussians next to
    ordinary ones (hundreds of rows per Gaussian: the projection backward's cooperative sums downstream)."""
    out = []
    sc, cam = case(14_000, 96, 64, seed=5)
    sc.opa += 1.5
    out.append(("deep_saturating", sc, cam))
    for n in (1, 15, 17, 63, 65, 1025):
        sc, cam = case(n, 96, 80, seed=100 + n)
        sc.pos[:, 2] = np.abs(sc.pos[:, 2]) + 1.0
        out.append((f"n{n}", sc, cam))
    sc, cam = case(20_000, 128, 96, seed=9)
    sc.opa[:] = -4.0
    out.append(("transparent", sc, cam))
    sc, cam = case(3_000, 352, 272, seed=31)
    big = [10, 11, 12, 700, 2999]
    sc.scale[big] = np.float32(3.0) * np.abs(sc.pos[big, 2:3]) / cam.focal_x * 40 * np.array([1.0, 0.55, 0.8], np.float32)
    sc.pos[big, :2] *= 0.05
    sc.pos[big, 2] = np.linspace(3.0, 8.0, len(big), dtype=np.float32)
    sc.opa[big] = -2.0
    out.append(("screen_filling", sc, cam))
    return out


def test_rgb_backward_row_layout_matches_oracle(gpu):
    """Round 5: raster_backward_rows_kernel (GS_FRAME_BWD_ROWS: lanes = 16 Gaussians x 4 pixel quads, transmittance and rho as
    DPP row scans, the opacity in the exponent, dead pixel rows left out) against the oracle's draw_backward + index sum +
    projection backward (gaussian.cu:440-803, splatter.py:604-613, gaussian.cu:1371-1576), element by element with the
    standard tolerances; and against the pixel-parallel kernel of the same build (another summation order: rel. L2)."""
    for k, (name, scene, cam) in enumerate(_rows_scenes()):
        strips = k % 2 == 0  # both binning variants (the row kernel only sees the sorted lists and the emission offsets)
        of = OracleFrame(scene, cam)
        gimg = np.random.default_rng(8).normal(size=of.image.shape).astype(np.float32)
        gimg, _ = of.robust_grad_image(gimg)
        ref, scale = of.backward(gimg, with_scale=True)
        got = {}
        for rows in (True, False):
            params = to_torch(scene, gpu, requires_grad=True)
            r = FrameRenderer(gpu, max_pairs=max(len(of.ids) + 64, 256), training=True, auto_grow=False, bwd_rows=rows,
                              force_strips=strips)
            img = r.render(*params, cam)
            assert bool(r._frame.flags & 64) == rows and r.binning_variant() == ("strip" if strips else "table")
            img.backward(torch.from_numpy(gimg).to(gpu))
            got[rows] = [t.grad.cpu().numpy() for t in params]
        assert_grads_close(got[True], ref, scale, f"row layout, {name}")
        for a, b, t in zip(got[True], got[False], ("pos", "quat", "scale", "opa", "rgb")):
            den = np.linalg.norm(b.astype(np.float64)) + 1e-300
            assert np.linalg.norm(a.astype(np.float64) - b) / den < 2e-5, (name, t)
            culled = of.mask == 0
            assert np.abs(a[culled]).max(initial=0.0) == 0.0, (name, t)


def test_row_layout_kernel_follows_the_saturated_bucket_statistic(gpu):
    """Which rgb backward kernel runs is the caller's decision (GS_FRAME_BWD_ROWS); FrameRenderer takes it from the share of
    the backward's buckets that belong to saturated tiles -- the upper half of the `buckets` counter, read back with the
    frame's other counters: an opaque scene (every tile's pixels saturate long before its list ends) switches the row
    layout on from the next frame, a transparent one (every list composited to its end) never does, bwd_rows=False
    never switches, and a renderer that goes from the first scene to the second switches off again."""
    dense, cam = case(60_000, 128, 96, seed=3)
    dense.opa += 3.0
    thin, _ = case(20_000, 128, 96, seed=9)
    thin.opa[:] = -4.0
    g = torch.from_numpy(np.random.default_rng(1).normal(size=(96, 128, 3)).astype(np.float32)).to(gpu)

    def step(r, scene):
        params = to_torch(scene, gpu, requires_grad=True)
        img = r.render(*params, cam)
        flag = bool(r._frame.flags & 64)
        img.backward(g)
        st = r.stats()  # (synchronises; the trainer reads the same counters asynchronously)
        return flag, st

    r = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=False)
    flag, st = step(r, dense)
    assert not flag and st.buckets > 0 and st.saturated_buckets > 0.9 * st.buckets and r._bwd_rows_seen
    flag, st = step(r, dense)
    assert flag  # from the second frame on
    flag, st = step(r, thin)
    assert flag and st.saturated_buckets < 0.1 * st.buckets and not r._bwd_rows_seen  # (this frame still ran flagged)
    flag, _ = step(r, thin)
    assert not flag
    never = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=False, bwd_rows=False)
    assert [step(never, dense)[0] for _ in range(3)] == [False, False, False]


# ------------------------------------------------------------------ BASELINE.json full sizes
@pytest.fixture(scope="module")
def cfg2_frame(gpu):
    """BASELINE.json configs[1]: 376,467 Gaussians at 1920x1080 (the bench workload)."""
    from gs_scene import CONFIGS

    n, W, H, use_sh = CONFIGS["cfg2"]
    scene, cam = make_scene(n, W, H, seed=2023, use_sh=use_sh), make_camera(W, H)
    params = to_torch(scene, gpu)
    out = {}
    for mode in (0, 1, 2):
        r = FrameRenderer(gpu, max_pairs=1_300_000, auto_grow=False, sort_mode=mode)
        img, _ = r.forward(*params, cam)
        v = r.debug_views()
        out[mode] = dict(img=img.cpu().numpy(), keys=v["sorted_keys"].cpu().numpy().view(np.uint64),
                         ids=v["sorted_ids"].cpu().numpy(), ranges=v["tile_ranges"].cpu().numpy(), stats=r.stats())
    return scene, cam, out


def test_full_size_sortedness_and_mode_equivalence(cfg2_frame):
    """Size-independent properties at the headline size: keys ascending, (key, id) strictly ascending
    (ties resolved by Gaussian index), tile ranges partition the list, and the three sort algorithms
    (six LSD passes / tile-bit passes + per-tile LDS sort / LDS counting sort + per-tile LDS sort) give the identical list and image."""
    _, _, out = cfg2_frame
    a, b = out[0], out[1]
    assert a["stats"].pairs == b["stats"].pairs == 1_088_150 and a["stats"].visible == 296_317
    k, i = b["keys"], b["ids"].astype(np.uint64)
    assert np.all(k[1:] >= k[:-1])
    comp_hi, comp_lo = k[1:] > k[:-1], i[1:] > i[:-1]
    assert np.all(comp_hi | ((k[1:] == k[:-1]) & comp_lo))
    tiles = (k >> np.uint64(32)).astype(np.int64)
    r = b["ranges"]
    cnt = np.bincount(tiles, minlength=len(r))
    assert np.array_equal(r[:, 1] - r[:, 0], cnt)
    nz = cnt > 0
    assert np.array_equal(r[nz, 0], (np.cumsum(cnt) - cnt)[nz])
    for other in (a, out[2]):
        assert np.array_equal(other["keys"], b["keys"]) and np.array_equal(other["ids"], b["ids"])
        assert np.array_equal(other["ranges"], b["ranges"])
        assert np.array_equal(other["img"], b["img"])


def test_full_size_forward_matches_oracle(cfg2_frame):
    """The whole cfg2 frame against the C oracle (a few seconds of CPU): pair list bit-exact, image 5e-5."""
    scene, cam, out = cfg2_frame
    of = OracleFrame(scene, cam)
    assert np.array_equal(out[1]["keys"], of.keys) and np.array_equal(out[1]["ids"], of.ids)
    err = np.abs(out[1]["img"] - of.image)
    assert err.max() < IMG_ATOL, err.max()


def test_full_size_backward_properties(gpu):
    """cfg2-size backward: gradients are finite, zero for culled Gaussians, bitwise repeatable, and
    linear in dL/dimage (g(2w) == 2 g(w): every operation is a product with the upstream gradient or a
    sum of such products, and scaling by 2 commutes with fp32 rounding outside the subnormal range)."""
    from gs_scene import CONFIGS

    n, W, H, use_sh = CONFIGS["cfg2"]
    scene, cam = make_scene(n, W, H, seed=2023, use_sh=use_sh), make_camera(W, H)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1_300_000, training=True, auto_grow=False)
    w = torch.randn(H, W, 3, device=gpu)
    r.forward(*params, cam)
    g1 = [t.clone() for t in r.backward(w)]
    r.forward(*params, cam)
    g1b = r.backward(w)
    r.forward(*params, cam)
    g2 = r.backward(2.0 * w)
    vis = r.debug_views()["rec_geom"][:, 2] != 0
    for a, b, c in zip(g1, g1b, g2):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
        # exact except where a partial sum is subnormal for w but normal for 2w (flushed vs kept)
        d = (2.0 * a - c).abs()
        assert float(d.max()) <= 1e-6 * float(c.abs().max()), (int((d > 0).sum()), float(d.max()))
        assert float((d > 0).float().mean()) < 1e-3, int((d > 0).sum())
        assert float(a[~vis].abs().max()) == 0.0
        assert float(a[vis].abs().max()) > 0.0


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3", "cfg4", "cfg4_deg3", "cfg5_yaw35", "cfg5_yaw35_rows"])
def test_full_size_backward_matches_oracle(gpu, cfg):
    """BASELINE.json configs[1], [2] (376,467 / 506,627 Gaussians, 1080p, rgb logits), [3] (2.4 M Gaussians, 1080p,
    SH: the reference's degree 2, and "cfg4_deg3": the degree 3 -- 48 coefficients, 115 M of them -- that configs[3]
    names) and the 8th view of configs[4] ("cfg5_yaw35": the 2.4 M scene, rgb logits, camera yawed by 35 degrees) at
    FULL size: all five parameter gradients of gs_frame_backward against the oracle's draw_backward
    (gaussian.cu:440-803) + index-backward sum (splatter.py:604-613) + projection backward (gaussian.cu:1371-1576),
    element by element.  dL/dimage is that of an L1 loss against a grey target, zeroed on the pixels whose stop
    decision is not robust in fp32 (counted: below 0.2 % of the image).
    The oracle's loops run on every host core (OpenMP; ~10 s for cfg2 / cfg3, about a minute for cfg4 on 8 cores)."""
    from gs_scene import CONFIGS

    base, _, variant = cfg.partition("_")
    rows = variant.endswith("_rows")  # "cfg5_yaw35_rows": the same view with the row-layout rgb kernel (GS_FRAME_BWD_ROWS)
    variant = variant[:-5] if rows else variant
    n, W, H, use_sh = CONFIGS[base]
    deg = 3 if variant == "deg3" else 2
    scene = make_scene(n, W, H, seed=2023, use_sh=use_sh, sh_degree=deg)
    cam = make_camera(W, H, yaw_deg=35.0 if variant == "yaw35" else 0.0)
    of = OracleFrame(scene, cam)
    gimg = (np.sign(of.image - 0.5) / of.image.size).astype(np.float32)
    gimg, n_masked = of.robust_grad_image(gimg)  # zero on the few pixels whose stop decision is not robust in fp32
    assert n_masked < 0.002 * W * H, (n_masked, W * H)
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    assert params[4].shape[1] == (3 * (deg + 1) ** 2 if use_sh else 3)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False, bwd_rows=rows)
    img = r.render(*params, cam)
    assert r.stats().pairs == len(of.ids)
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < IMG_ATOL
    assert bool(r._frame.flags & 64) == rows
    img.backward(torch.from_numpy(gimg).to(gpu))
    got = [t.grad.cpu().numpy() for t in params]
    report = assert_grads_close(got, ref, scale, cfg)
    print(cfg, f"pixels with dL/dimage masked: {n_masked} ({100.0 * n_masked / (W * H):.3f} %);",
          "gradient parity (worst err/tol, fraction within rtol alone, rel. L2, worst pure relative error above "
          "1e-6 of the maximum):", report)
    # calibrated, oracle-scale-free statement: against a DOUBLE-precision evaluation of the same chain, the HIP
    # kernels' relative error is -- quantile by quantile, median to maximum -- within CALIB_K x the error of the
    # reference's own fp32 arithmetic (the oracle's fp32 terms; tests/test_grad_calibration.py shows its error
    # distribution is the reference kernels')
    _, truth = of.backward_f64(gimg)
    calib = assert_error_no_worse_than(got, truth, ref, cfg)
    for name, (qh, qr) in calib.items():
        print(f"CALIB {cfg} {name}: hip", ["%.2e" % v for v in qh], "reference arithmetic", ["%.2e" % v for v in qr])
    culled = of.mask == 0
    for t in params:
        assert float(t.grad[torch.from_numpy(culled).to(gpu)].abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025])
@pytest.mark.parametrize("force_strips", [True, False])
def test_frame_forward_backward_at_block_boundaries(gpu, n, force_strips):
    """Gaussian counts around the 64-lane wave and the 256-thread block: list, image and gradients against the oracle
    (both the strip and the size-selected table variant of the binning)."""
    scene, cam = case(n, 96, 80, seed=100 + n)
    scene.pos[:, 2] = np.abs(scene.pos[:, 2]) + 1.0  # in front of the camera: tiny scenes should not be all culled
    of = OracleFrame(scene, cam)
    params = to_torch(scene, gpu, requires_grad=True)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False, force_strips=force_strips)
    img = r.render(*params, cam)
    assert r.binning_variant() == ("strip" if force_strips else "table")
    st, v = r.stats(), r.debug_views()
    assert (st.visible, st.pairs) == (int(of.mask.sum()), len(of.ids))
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)
    assert np.array_equal(v["visible"].cpu().numpy(), of.mask.astype(bool))
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < IMG_ATOL
    gimg = np.random.default_rng(n).normal(size=of.image.shape).astype(np.float32)
    gimg, _ = of.robust_grad_image(gimg)
    ref, scale = of.backward(gimg, with_scale=True)
    img.backward(torch.from_numpy(gimg).to(gpu))
    assert_grads_close([t.grad.cpu().numpy() for t in params], ref, scale, f"n={n}")


def test_binning_variant_is_chosen_by_scene_size(gpu):
    """sort_mode 2 without a variant flag: the table variant below GS_STRIP_AUTO_MIN_N Gaussians (131,072), the strip
    variant from there on; GS_FRAME_STRIP_BIN / GS_FRAME_TABLE_BIN override.  The lists are the same either way."""
    W, H = 320, 240
    cam = make_camera(W, H)
    ids = {}
    for n, expect in ((20_000, "table"), (131_072, "strip")):
        scene = make_scene(n, W, H, seed=3)
        params = to_torch(scene, gpu)
        for kw, want in ((dict(force_strips=False), expect), (dict(force_strips=True), "strip"),
                         (dict(table_bin=True), "table")):
            r = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False, **kw)
            img, _ = r.forward(*params, cam)
            assert r.binning_variant() == want, (n, kw, r.binning_variant())
            got = (r.debug_views()["sorted_ids"].clone(), img.clone())
            if n in ids:
                assert torch.equal(got[0], ids[n][0]) and torch.equal(got[1], ids[n][1])
            ids[n] = got


def test_full_size_2p4M_forward_matches_oracle(gpu):
    """BASELINE.json configs[4] geometry (2.4 M Gaussians, 1080p, no SH: the >= 160 FPS target scene): the whole
    frame against the C oracle -- 6.95 M (tile, depth, id) pairs bit-exact, image to IMG_ATOL (~30 s of CPU)."""
    from gs_scene import CONFIGS

    n, W, H, use_sh = CONFIGS["cfg5"]
    scene, cam = make_scene(n, W, H, seed=2023, use_sh=use_sh), make_camera(W, H)
    params = to_torch(scene, gpu)
    of = OracleFrame(scene, cam)
    for variant in ({}, dict(table_bin=True)):  # the strip (default) and the table variant of the binning
        r = FrameRenderer(gpu, max_pairs=7_600_000, auto_grow=False, **variant)
        img, _ = r.forward(*params, cam)
        st, v = r.stats(), r.debug_views()
        assert (st.visible, st.pairs, st.overflow) == (1_887_982, 6_950_364, 0)
        assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys)
        assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)
        err = np.abs(img.cpu().numpy() - of.image)
        assert err.max() < IMG_ATOL, err.max()
        if not variant:
            # the next frame of the same renderer is occlusion-culled (strip variant): 71 % of this scene's pairs lie behind
            # their tile's stop and are no longer emitted; the image is the same bit for bit
            img2, _ = r.forward(*params, cam)
            st2 = r.stats()
            assert r._frame.flags & 256 and not st2.cull_fallback and st2.pairs < 0.45 * st.pairs, st2
            assert torch.equal(img2, img)
            print("cfg5 occlusion cull: pairs emitted", st2.pairs, "of", st.pairs)
        del r


def test_full_size_2p4M_sh_forward_backward_properties(gpu):
    """BASELINE.json configs[3] (2.4 M Gaussians, 1080p, SH, forward + backward) through size-independent
    properties: same pair list as the no-SH scene of the same geometry, finite image and gradients, bitwise
    repeatable backward, zero gradient for culled Gaussians, linear in dL/dimage."""
    from gs_scene import CONFIGS

    n, W, H, use_sh = CONFIGS["cfg4"]
    scene, cam = make_scene(n, W, H, seed=2023, use_sh=use_sh), make_camera(W, H)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=7_600_000, training=True, auto_grow=False)
    w = torch.randn(H, W, 3, device=gpu)
    img, _ = r.forward(*params, cam)
    assert r.stats().pairs == 6_950_364 and bool(torch.isfinite(img).all())
    g1 = [t.clone() for t in r.backward(w)]
    r.forward(*params, cam)
    g1b = r.backward(w)
    r.forward(*params, cam)
    g2 = r.backward(2.0 * w)
    vis = r.debug_views()["rec_geom"][:, 2] != 0
    assert g1[4].shape == (n, 27)
    for a, b, c in zip(g1, g1b, g2):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        assert float((2.0 * a - c).abs().max()) <= 1e-6 * float(c.abs().max())
        assert float(a[~vis].abs().max()) == 0.0 and float(a[vis].abs().max()) > 0.0


@pytest.mark.parametrize("kind", ["nan_pos", "inf_pos", "zero_quat", "nan_scale", "huge_scale", "zero_scale", "neg_z",
                                  "nan_opa", "nan_rgb", "inf_opa"])
def test_frame_degenerate_inputs(gpu, kind):
    """Non-finite / degenerate parameters must neither hang nor corrupt anything else: the pair list still
    equals the oracle's (NaN comparisons behave like the reference's) and so does the image -- including WHICH pixels
    go NaN: a NaN opacity or colour reaches the pixels that are still live when its Gaussian comes up and leaves the
    finished ones alone, as in the reference, which `break`s before it evaluates the Gaussian (gaussian.cu:906); the
    kernel multiplies alpha and T with v_mul_legacy_f32 (0 x NaN = 0) and moves a NaN colour into the opacity (so a
    NaN in ONE colour channel turns all three channels of the live pixels NaN, not just that one: compared per pixel)."""
    scene, cam = case(6_000, 160, 112, seed=3)
    idx = np.random.default_rng(1).choice(6_000, 60, replace=False)
    if kind == "nan_pos":
        scene.pos[idx, 0] = np.nan
    elif kind == "inf_pos":
        scene.pos[idx, 1] = np.inf
    elif kind == "zero_quat":
        scene.quat[idx] = 0
    elif kind == "nan_scale":
        scene.scale[idx, 2] = np.nan
    elif kind == "huge_scale":
        scene.scale[idx] = 1e6
    elif kind == "zero_scale":
        scene.scale[idx] = 0
    elif kind == "neg_z":
        scene.pos[idx, 2] = -1
    elif kind == "nan_opa":
        scene.opa[idx] = np.nan
    elif kind == "inf_opa":
        scene.opa[idx] = np.inf  # sigmoid = 1: alpha = G exactly, a legal fully opaque Gaussian
    elif kind == "nan_rgb":
        scene.rgb[idx, 1] = np.nan
    if kind in ("nan_opa", "nan_rgb"):
        scene.opa += 3.0  # opaque scene: most pixels are finished long before the list ends
    with np.errstate(all="ignore"):
        of = OracleFrame(scene, cam)
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True)
    params = to_torch(scene, gpu, requires_grad=True)
    img = r.render(*params, cam)
    st = r.stats()
    assert st.overflow == 0 and st.pairs == len(of.ids)
    v = r.debug_views()
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids)
    got = img.detach().cpu().numpy()
    finite = np.isfinite(of.image)
    if kind in ("nan_opa", "nan_rgb"):
        assert 0.02 < 1.0 - finite.mean() < 0.98  # the case really separates live from finished pixels
    if kind == "nan_rgb":
        finite = np.repeat(finite.all(axis=2, keepdims=True), 3, axis=2)
    assert np.array_equal(np.isfinite(got), finite)
    assert np.abs(got[finite] - of.image[finite]).max() < IMG_ATOL
    img.sum().backward()  # must terminate; gradients of untouched Gaussians stay finite
    torch.cuda.synchronize()
    if kind in ("huge_scale", "zero_scale", "neg_z"):
        assert all(bool(torch.isfinite(t.grad).all()) for t in params)


def test_frame_async_growth(gpu):
    """auto_grow="async": the first frame (and every inference frame) is capacity-checked synchronously and redone in
    a larger workspace -- never returned empty; later TRAINING frames only copy their counters to pinned memory.  If
    such a frame overflows all the same (here: the capacity is cut behind the renderer's back), it is rendered
    empty, counted and reported, and the next frames are complete again."""
    scene, cam = case(10_000, 128, 128)
    of = OracleFrame(scene, cam)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) // 3, auto_grow="async", training=True)
    first = r.forward(*params, cam)[0].clone()
    assert r.max_pairs >= len(of.ids) and np.abs(first.cpu().numpy() - of.image).max() < IMG_ATOL
    assert r.overflowed_frames == 0
    r.max_pairs = len(of.ids) // 3  # as if the scene had grown three-fold between two frames
    imgs = []
    for _ in range(4):
        imgs.append(r.forward(*params, cam)[0].clone())
        if len(imgs) == 1:
            assert r.last_frame_overflowed(wait=True)
        torch.cuda.synchronize()  # only so that the test is deterministic: the copy has landed before the next frame
    assert float(imgs[0].abs().max()) == 0.0  # sort_mode 2 renders an overflowed frame empty instead of truncated
    assert r.overflowed_frames == 1 and r.max_pairs >= len(of.ids)
    assert np.abs(imgs[-1].cpu().numpy() - of.image).max() < IMG_ATOL
    # an inference frame is never returned truncated, whatever the capacity was
    r.max_pairs = len(of.ids) // 3
    img = r.forward(*params, cam, training=False)[0]
    assert np.abs(img.cpu().numpy() - of.image).max() < IMG_ATOL and r.overflowed_frames == 1


def test_async_counters_lag_is_bounded(gpu):
    """auto_grow="async": the host never issues more than ASYNC_COUNTER_LAG frames beyond the frame whose counters are still on
    their way (round 5: a Python loop runs hundreds of frames ahead of the device otherwise, the growth a frame asked for
    arrives hundreds of frames late and frames overflow -- are rendered empty, their steps skipped -- without anybody looking;
    tools/fused_adam_bisect.py).  A scene whose pair count doubles behind the renderer's back is picked up within that many
    frames although nothing in the loop synchronises."""
    scene, cam = case(10_000, 128, 128)
    of = OracleFrame(scene, cam)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) * 2, auto_grow="async", training=True)
    r.forward(*params, cam)
    lag = FrameRenderer.ASYNC_COUNTER_LAG
    assert 1 <= lag <= 64
    r.max_pairs = len(of.ids) // 2  # as if the scene had doubled: every frame overflows until the counters are looked at
    frames = 0
    while r.max_pairs < len(of.ids) and frames < 10 * lag:
        r.forward(*params, cam)
        frames += 1
        assert r._async_event is None or r._frame_serial - r._async_serial <= lag
    assert frames <= lag + 2 and r.max_pairs >= len(of.ids), (frames, r.max_pairs, len(of.ids))
    img = r.forward(*params, cam)[0]
    assert np.abs(img.cpu().numpy() - of.image).max() < IMG_ATOL


def test_c_abi_client_without_torch(gpu, tmp_path):
    """examples/abi_demo.cpp links libgs_amd.so and the HIP runtime only (no torch, no Python): the same scene
    rendered through that client and through FrameRenderer gives bit-identical images and counters."""
    import os
    import struct
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "abi_demo")
    if not os.path.exists(exe):
        pytest.skip("examples/abi_demo not built (python __graft_entry__.py)")
    libs = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libgs_amd.so" in libs and "torch" not in libs and "python" not in libs
    W, H = 333, 201
    scene, cam = case(9_000, W, H, seed=23)
    scene_file, out_file = tmp_path / "scene.bin", tmp_path / "out.bin"
    with open(scene_file, "wb") as f:
        f.write(struct.pack("<3i3f", scene.n, W, H, cam.focal_x, cam.focal_y, cam.near))
        f.write(np.asarray(cam.rot, np.float32).tobytes() + np.asarray(cam.tran, np.float32).tobytes())
        for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    p = subprocess.run([exe, str(scene_file), str(out_file)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    raw = open(out_file, "rb").read()
    visible, pairs = struct.unpack_from("<2q", raw, 0)
    image = np.frombuffer(raw, np.float32, W * H * 3, 16).reshape(H, W, 3)
    r = FrameRenderer(gpu, max_pairs=8 * scene.n + 4096, auto_grow=False)
    ref, _ = r.forward(*to_torch(scene, gpu), cam)
    st = r.stats()
    assert (visible, pairs) == (st.visible, st.pairs)
    assert np.array_equal(image, ref.cpu().numpy())
    assert "culled by the library 0" in p.stdout and "image identical" in p.stdout  # (9,000 Gaussians: the flag is ignored)
    # the client's second frame carries GS_FRAME_OCCLUSION_CULL: on a scene of the strip variant's size, opaque, the library
    # culls it (fewer pairs emitted), and the client itself checks that the image is the first frame's bit for bit
    scene2, cam2 = case(150_000, W, H, seed=29)
    scene2.opa += 3.0
    with open(scene_file, "wb") as f:
        f.write(struct.pack("<3i3f", scene2.n, W, H, cam2.focal_x, cam2.focal_y, cam2.near))
        f.write(np.asarray(cam2.rot, np.float32).tobytes() + np.asarray(cam2.tran, np.float32).tobytes())
        for a in (scene2.pos, scene2.quat, scene2.scale, scene2.opa, scene2.rgb):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    p2 = subprocess.run([exe, str(scene_file), str(out_file)], capture_output=True, text=True, timeout=120)
    assert p2.returncode == 0, p2.stderr
    assert "culled by the library 1" in p2.stdout and "fell back 0, image identical" in p2.stdout, p2.stdout
    import re
    emitted, full = map(int, re.search(r"pairs emitted (\d+) of (\d+)", p2.stdout).groups())
    assert 0 < emitted < 0.7 * full


def test_frame_forward_is_graph_capturable(gpu):
    """No allocation, host synchronisation or lazy initialisation inside gs_frame_forward once it has run: the
    launch sequence can be captured into a hipGraph (torch.cuda.graph) and replayed.  (Measured on MI355X: replay
    is NOT faster than eager launches -- 21 k vs 24 k FPS at 10 k Gaussians -- the per-kernel dependency latency
    is on the GPU side; see DESIGN.md.)"""
    scene, cam = case(20_000, 320, 208, seed=23)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=200_000, auto_grow=False)
    want = r.forward(*params, cam)[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.forward(*params, cam)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        img, _ = r.forward(*params, cam)
    for _ in range(3):
        img.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(img, want)
    # new parameter VALUES in the same buffers are picked up by the replay
    params[3].add_(0.7)
    want2 = r.forward(*params, cam)[0].clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(img, want2) and not torch.equal(want, want2)


def test_training_forward_followed_by_inference_forward_on_the_same_workspace(gpu):
    """A training forward leaves work on the library's side stream (zero-fill of the gradient rows, bucket list for a
    backward that may never come).  The next forward on the same workspace -- with the inference layout, where
    those bytes hold other buffers -- must wait for it: alternate the two many times and compare with a renderer of
    its own."""
    scene, cam = case(40_000, 640, 400, seed=37)
    params = to_torch(scene, gpu)
    want = FrameRenderer(gpu, max_pairs=400_000, auto_grow=False).forward(*params, cam)[0].clone()
    r = FrameRenderer(gpu, max_pairs=400_000, training=True, auto_grow=False)
    for _ in range(25):
        r.forward(*params, cam, training=True)
        img, _ = r.forward(*params, cam, training=False)
        assert torch.equal(img, want)
    # and the backward of a training forward still gets its zeroed rows after such a sequence
    g = torch.randn(400, 640, 3, device=gpu)
    r.forward(*params, cam, training=True)
    a = [t.clone() for t in r.backward(g)]
    r.forward(*params, cam, training=False)
    r.forward(*params, cam, training=True)
    b = r.backward(g)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_ray_basis_is_built_when_an_sh_frame_follows_an_rgb_frame_of_the_same_camera(gpu):
    """The per-camera constants are cached per camera, and the ray basis (only read by the SH colours) is left out of
    the rgb entry: an SH frame of the same renderer and camera must not pick that entry up.  Also a camera that moves
    every frame (no cache hit at all) renders what a fresh renderer renders."""
    scene, cam = case(3000, 128, 96, seed=51)
    sh_scene, _ = case(3000, 128, 96, seed=51, use_sh=True)
    rgb_params, sh_params = to_torch(scene, gpu), to_torch(sh_scene, gpu)
    want = FrameRenderer(gpu, max_pairs=1 << 16).forward(*sh_params, cam)[0].clone()
    r = FrameRenderer(gpu, max_pairs=1 << 16)
    r.forward(*rgb_params, cam)
    got = r.forward(*sh_params, cam)[0]
    assert torch.equal(got, want)
    assert np.abs(got.cpu().numpy() - OracleFrame(sh_scene, cam).image).max() < IMG_ATOL
    for yaw in (-3.0, 0.5, 2.0):
        moved = make_camera(128, 96, yaw_deg=yaw)
        moved.tran = cam.tran
        a = r.forward(*sh_params, moved)[0]
        b = FrameRenderer(gpu, max_pairs=1 << 16).forward(*sh_params, moved)[0]
        assert torch.equal(a, b)
