"""GPU tier of the depth / alpha maps' GRADIENTS in every backward regime (raster_aux_backward_kernel<3 | 27 | 48>, the depth
term of the projection backward): the only backward compositing kernel RGB-D training, pose refinement on depth and
render_aux autograd execute, held to the image backward's standard.

Yardstick: tests/gs_testutil.OracleFrame.aux_backward (the oracle with the maps posed as colours, checked on the CPU tier by
tests/test_aux_host.py) and aux_backward_f64.  Every case goes through FrameRenderer / the C ABI, asserts the pair count
and the image / alpha / depth maps (test_gpu_aux.check_maps), then runs the backward THREE ways into NaN-filled
destinations -- all three gradients; the maps only; the depth map only (which isolates the extra row of the staged line and
the dep_i factor that the image term otherwise dominates) -- and compares with assert_grads_close at the project's defaults
(GRAD_RTOL, GRAD_KAPPA, GRAD_L2) unless the mirrored image test states others; culled Gaussians get exact zeros.  Every
case asserts a precondition on the ORACLE's data, so that a scene cannot drift out of its regime unnoticed, and caps the
pixels masked for a non-robust stop decision: below 0.5 % of a small frame, 0.2 % of a full-size one.
"""
import hashlib

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene, make_trained_like_scene
from gs_testutil import (CALIB_K, GRAD_L2, OracleFrame, assert_error_no_worse_than, assert_grads_close, aux_case,
                         depth_loss_f64, robust_aux_grads, saturated_share, to_torch)
from test_gpu_aux import IMG_ATOL, _dense, check_maps

pytestmark = pytest.mark.gpu

NAMES = ("pos", "quat", "scale", "opa", "rgb")
COLOURS = [(False, 2), (True, 2), (True, 3)]
COLOUR_IDS = ["rgb", "sh2", "sh3"]
WAYS = ("all", "maps", "depth")
SMALL_CAP, FULL_CAP = 0.005, 0.002  # masked pixels, as a share of the image


def _t(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _way(way, gimg, gd, ga):
    return {"all": (gimg, gd, ga), "maps": (None, gd, ga), "depth": (None, gd, None)}[way]


def _forward(gpu, of, scene, cam, r_kw, grow=False, img_atol=IMG_ATOL, repeat=1, check=True):
    """A training aux frame of ``scene``: pair count and pair list equal to the oracle's, image / alpha / depth within
    check_maps' standard.  -> (renderer, depth, alpha)"""
    params = to_torch(scene, gpu)
    if grow:  # "dist" frames: the rows cover the bounding squares; the workspace grows to their sum first
        r = FrameRenderer(gpu, max_pairs=max(len(of.ids), 64), training=True, auto_grow=True, **r_kw)
        r.forward(*params, cam, aux=True)
        r.auto_grow = False
    else:
        r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=True, auto_grow=False, **r_kw)
    for _ in range(repeat):  # (repeat = 2: the second frame carries the flags the first frame's counters asked for)
        image, padded, depth, alpha = r.forward(*params, cam, aux=True)
        st = r.stats()
    assert r._frame.flags & _lib.GS_FRAME_AUX
    assert st.overflow == 0 and st.pairs == len(of.ids) and st.visible == int(of.mask.sum())
    if len(of.ids):
        assert np.array_equal(r.debug_views()["sorted_ids"].cpu().numpy(), of.ids), "pair list differs from the oracle's"
    if check:
        err = float(np.abs(image.cpu().numpy() - of.image).max())
        assert err < img_atol, err
        check_maps(of, depth, alpha, r._aux_keep[2])
    return r, depth, alpha


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / (np.linalg.norm(np.asarray(b, np.float64)) + 1e-300))


# The maps' gradients do not depend on the colour model: the three colour parametrisations of a case share geometry,
# opacities, camera and (gd, ga), so the oracle's answers for the ways without dL/dimage are computed once per such
# input (keyed by a digest of everything they depend on) and re-shaped to the colour dimension at hand.
_MAPS_CACHE = {}
OWN_L2_CEILING = 1e-4  # the fp32 oracle's own relative L2 against fp64 in the calibrated cases (measured: up to 5.4e-5)


def _maps_answers(of, d, a, f64):
    sc, cam = of.scene, of.cam
    h = hashlib.sha1()
    for x in (sc.pos, sc.quat, sc.scale, sc.opa, cam.rot, cam.tran, of.ids, of.accum, d, a):
        h.update(b"-" if x is None else np.ascontiguousarray(x).tobytes())
    h.update(repr((cam.width, cam.height, cam.focal_x, cam.focal_y, of.scale_activation, bool(f64))).encode())
    key = h.hexdigest()
    if key not in _MAPS_CACHE:
        if len(_MAPS_CACHE) > 16:
            _MAPS_CACHE.clear()
        _MAPS_CACHE[key] = of.aux_backward_f64(None, d, a) if f64 else of.aux_backward(None, d, a)
    zc = np.zeros(sc.rgb.shape, np.float64 if f64 else np.float32)
    if f64:
        return dict(_MAPS_CACHE[key], rgb=zc)
    ref, scale = _MAPS_CACHE[key]
    return dict(ref, rgb=zc), dict(scale, rgb=np.zeros(sc.rgb.shape))


def _backward_three_ways(gpu, r, of, scene, gimg, gd, ga, what, tol=None, subset=None, ways=WAYS, refs=None,
                         calibrated=None):
    """gs_frame_backward of the current aux frame against OracleFrame.aux_backward, each way into NaN-filled buffers.
    ``refs``: a dict that keeps the oracle's answers per way (two renderers compared on one scene share them).
    ``calibrated``: for the regimes in which the fp32 ORACLE itself does not meet the defaults against the double
    evaluation (stated, with the measured figures, where it is used); what the reference arithmetic achieves on the
    scene, never the kernel's output, sets the bound, and that achievement is itself capped (OWN_L2_CEILING):
      "l2":   element-wise the defaults against the oracle; the relative L2 per tensor, taken against
              aux_backward_f64, within max(GRAD_L2, CALIB_K x the oracle's own);
      "full": that L2 bound, and in place of the element-wise criterion the relative error against aux_backward_f64 quantile
              by quantile within CALIB_K (CALIB_K_MAX at the maximum) of the oracle's own (assert_error_no_worse_than,
              the statement of the full-size tests)."""
    assert calibrated in (None, "l2", "full")
    tol = dict(tol or {})
    refs = {} if refs is None else refs
    culled = ~of.mask.astype(bool)
    reports = {}
    for way in ways:
        gi, d, a = _way(way, gimg, gd, ga)
        if way not in refs:
            refs[way] = of.aux_backward(gi, d, a) if gi is not None else _maps_answers(of, d, a, False)
        ref, scale = refs[way]
        if calibrated and ("f64", way) not in refs:
            truth = of.aux_backward_f64(gi, d, a) if gi is not None else _maps_answers(of, d, a, True)
            own = {k: _rel_l2(ref[k], truth[k]) for k in NAMES}
            assert max(own.values()) <= OWN_L2_CEILING, (what, way, "the oracle's own relative L2 against fp64", own)
            refs["f64", way] = (truth, own)
        out = tuple(torch.full_like(p, float("nan")) for p in r._keep[:5])
        r.backward(_t(gpu, gi), out=out, grad_depth=_t(gpu, d), grad_alpha=_t(gpu, a))
        got = [x.cpu().numpy() for x in out]
        for x in got:
            assert np.isfinite(x).all(), (what, way, "a destination element was not written")
            assert np.all(x[culled] == 0), (what, way, "culled Gaussians must get exact zeros")
        if way != "all":
            assert np.all(got[4] == 0), (what, way, "the maps carry no colour gradient")
        if calibrated != "full":
            rep = assert_grads_close(got, ref, scale, f"{what} [{way}]", **dict(tol, l2=np.inf) if calibrated else tol)
            print(f"AUXBWD {what} [{way}]:", {k: (v[0], "%.2e" % v[2]) for k, v in rep.items()},
                  "(worst err/tol, rel. L2)")
        if calibrated:
            truth, own = refs["f64", way]
            l2 = {k: _rel_l2(g, truth[k]) for g, k in zip(got, NAMES)}
            print(f"AUXBWD {what} [{way}], rel. L2 against fp64:", {k: "%.2e" % v for k, v in l2.items()},
                  "the fp32 oracle's own:", {k: "%.2e" % v for k, v in own.items()})
            for k in NAMES:
                assert l2[k] <= max(GRAD_L2, CALIB_K * own[k]), (what, way, k, "relative L2 error", l2[k], "oracle's", own[k])
        if calibrated == "full":
            calib = assert_error_no_worse_than(got, truth, ref, f"{what} [{way}]")
            for k, (qh, qr) in calib.items():
                print(f"CALIB aux {what} [{way}] {k}: hip", ["%.2e" % v for v in qh], "reference arithmetic",
                      ["%.2e" % v for v in qr])
        assert any(np.abs(ref[k]).max() > 0 for k in ("pos", "opa")) or not len(of.ids)
        if subset is not None:
            idx, l2 = subset
            assert_grads_close([g[idx] for g in got], {k: v[idx] for k, v in ref.items()},
                               {k: v[idx] for k, v in scale.items()}, f"{what} [{way}], the workgroup-summed ones", l2=l2)
        reports[way] = (got, ref, scale)
    return reports


def _run(gpu, scene, cam, what, seed, of_kw=None, r_kw=None, tol=None, subset=None, grow=False, img_atol=IMG_ATOL,
         repeat=1, expect_masked=None, precondition=None):
    of = OracleFrame(scene, cam, **(of_kw or {}))
    if precondition is not None:
        precondition(of)
    gimg, gd, ga, n_masked = robust_aux_grads(of, seed)
    H, W = of.image.shape[:2]
    assert n_masked < SMALL_CAP * W * H, (what, n_masked, W * H)
    if expect_masked is not None:
        assert n_masked == expect_masked, (what, n_masked)
    r, _, _ = _forward(gpu, of, scene, cam, r_kw or {}, grow=grow, img_atol=img_atol, repeat=repeat)
    _backward_three_ways(gpu, r, of, scene, gimg, gd, ga, what, tol=tol, subset=subset)
    return of, r


def _lists(of):
    return np.diff(of.accum)


# ------------------------------------------------------------------------------------------- 1. translucent / half / deep
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("which", ["base", "deep"])
def test_translucent(gpu, which, use_sh, deg):
    """No pixel stops, every list is walked to its end, A < 1 everywhere: the state of a trained model, the only one in
    which the alpha map carries gradient and the (D, A) suffix is taken against a final A that is not 1.  "deep": lists of
    many buckets AND live: the deep-tiles scene needs opa -= 7 for that (oracle, measured: with -= 4 its lists of up to 1,873
    still saturate 77 % of the pixels and 2.5 % of them are masked; with -= 7 none saturates, mean alpha 0.62)."""
    scene, cam = aux_case(5000, 128, 96, seed=13, use_sh=use_sh, sh_degree=deg) if which == "base" else \
        aux_case(14_000, 96, 64, seed=5, use_sh=use_sh, sh_degree=deg)
    scene.opa -= np.float32(4.0 if which == "base" else 7.0)

    def pre(of):
        a = of.grid.crop(of.aux_maps()[:, :, 1:2])[:, :, 0]
        assert saturated_share(of) < 0.01 and 0.05 < float(a.mean()) < 0.95, (saturated_share(of), float(a.mean()))
        assert _lists(of).max() > (300 if which == "base" else 1000)

    _run(gpu, scene, cam, f"translucent {which} sh={use_sh} deg={deg}", 101, expect_masked=0, precondition=pre)


@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
def test_half_and_half(gpu, use_sh, deg):
    """Stopped and live pixels inside the same tiles and buckets (a fifth of the pixels saturates)."""
    scene, cam = aux_case(5000, 128, 96, seed=13, use_sh=use_sh, sh_degree=deg)
    scene.opa -= np.float32(2.0)

    def pre(of):
        assert 0.1 < saturated_share(of) < 0.5, saturated_share(of)

    _run(gpu, scene, cam, f"half and half sh={use_sh} deg={deg}", 103, precondition=pre)


@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("which", ["deep", "dense"])
def test_deep_saturating_tiles(gpu, which, use_sh, deg):
    """test_gpu_frame.py::test_frame_backward_sh_deep_saturating_tiles' scene and test_gpu_aux.py's _dense(): tiles many
    64-Gaussian buckets deep whose pixels all stop inside the list (the stop bucket's checkpoint, dead buckets behind)."""
    if which == "deep":
        scene, cam = aux_case(14_000, 96, 64, seed=5, use_sh=use_sh, sh_degree=deg)
        scene.opa += np.float32(1.5)
    else:
        scene, cam = _dense()
        if use_sh:
            scene, cam = make_scene(60_000, 192, 128, seed=3, use_sh=True, sh_degree=deg), make_camera(192, 128)
            scene.opa += 3.0

    def pre(of):
        assert _lists(of).max() > 300 and saturated_share(of) > 0.9, (_lists(of).max(), saturated_share(of))

    _run(gpu, scene, cam, f"deep saturating {which} sh={use_sh} deg={deg}", 105, precondition=pre)


# ------------------------------------------------------------------------------------------------------- 2. long lists
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("shift", [0.0, -10.0], ids=["opaque", "translucent"])
def test_long_lists_training(gpu, shift, use_sh, deg):
    """test_aux_forward_long_lists' scene -- lists of 30+ buckets, beyond the 2,048-pair window of the per-tile sort -- in a
    TRAINING frame, as it is and translucent, with GS_FRAME_LONG_LISTS forced (long_lists=True) and with the flags the
    renderer sets by itself from the first frame's counters (long_lists=None), both against one set of oracle answers: the
    aux frame composites without segments, so the maps are held to check_maps' standard and the gradients to the
    defaults.  Translucent here is opa -= 10 (oracle, measured: lists of ~15,000 still saturate 91 % of the pixels at
    -= 4, with 1.5 % of them masked; at -= 10 none saturates, mean alpha 0.62).

    Tolerances: chains of ~15,000 layers are beyond what fp32 delivers at the defaults, whoever walks them -- measured
    on the fp32 ORACLE against aux_backward_f64.  Opaque scene (99.6 % of the pixels saturated; the maps' gradient is a sum
    of differences of nearly equal numbers): element-wise inside the defaults, but relative L2 2.9e-5 (pos) / 4.9e-5
    (quat) / 4.7e-5 (scale) / 5.4e-5 (opa) for the maps alone, 1.2e-5 ... 2.6e-5 for the depth map alone, above GRAD_L2 =
    2e-5 itself: calibrated="l2".  Translucent scene: the oracle's worst element sits at 1.05 x (all) / 1.6 x (maps) /
    2.7 x (depth) the default element-wise tolerance against the double value, its relative L2 at 1.2e-5 ... 1.9e-5; and
    where the kernel differed most from the fp32 oracle (1.33 x the default tolerance) it was CLOSER to the double value
    (-0.00425870 against -0.00425910) than the oracle (-0.00426038): calibrated="full", the quantile statement of the
    full-size tests against the double evaluation."""
    scene = make_scene(120_000, 128, 96, seed=8, max_px_sigma=40.0, use_sh=use_sh, sh_degree=deg)
    cam = make_camera(128, 96)
    scene.opa += np.float32(shift)
    of = OracleFrame(scene, cam)
    assert _lists(of).max() > 2048, _lists(of).max()
    a = of.grid.crop(of.aux_maps()[:, :, 1:2])[:, :, 0]
    if shift:
        assert saturated_share(of) < 0.01 and 0.05 < float(a.mean()) < 0.95, (saturated_share(of), float(a.mean()))
    else:
        assert saturated_share(of) > 0.9
    gimg, gd, ga, n_masked = robust_aux_grads(of, 107)
    assert n_masked < SMALL_CAP * 128 * 96, n_masked
    refs = {}
    for long_lists in (True, None):
        r, _, _ = _forward(gpu, of, scene, cam, dict(long_lists=long_lists), repeat=1 if long_lists else 2)
        if long_lists:
            assert r._frame.flags & _lib.GS_FRAME_LONG_LISTS
        else:
            assert r._long_sort_seen and (r._frame.flags & _lib.GS_FRAME_LONG_SORT)
            assert bool(r._frame.flags & _lib.GS_FRAME_LONG_LISTS) == r._long_lists_seen
        print("AUXBWD long lists: longest", int(_lists(of).max()), "long_lists", long_lists, "flags", int(r._frame.flags))
        _backward_three_ways(gpu, r, of, scene, gimg, gd, ga,
                             f"long lists shift={shift} long_lists={long_lists} sh={use_sh} deg={deg}", refs=refs,
                             calibrated="full" if shift else "l2")


# ------------------------------------------------------------------------------------- 3. workgroup-summed Gaussians
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
def test_workgroup_summed_gaussians(gpu, use_sh, deg):
    """test_gpu_frame.py::test_frame_backward_screen_filling_gaussians' scene: Gaussians of more than 256 rows (`big`) and of
    65 - 256 rows (`mid`), whose per-pair rows -- the depth float of the staged line included -- are summed by the whole
    workgroup; a second comparison on those Gaussians alone with l2 = 1e-4, as there."""
    scene, cam = aux_case(3_000, 352, 272, seed=31, use_sh=use_sh, sh_degree=deg)
    big = [10, 11, 12, 700, 2999]
    scene.scale[big] = np.float32(3.0) * np.abs(scene.pos[big, 2:3]) / cam.focal_x * 40 * \
        np.array([1.0, 0.55, 0.8], np.float32)
    scene.pos[big, :2] *= 0.05
    scene.pos[big, 2] = np.linspace(3.0, 8.0, len(big), dtype=np.float32)
    scene.opa[big] = -2.0
    mid = [1500, 1501, 1503, 2200]
    scene.scale[mid] = np.float32(3.0) * np.abs(scene.pos[mid, 2:3]) / cam.focal_x * 13 * \
        np.array([1.0, 0.7, 0.85], np.float32)
    scene.pos[mid, :2] *= 0.3
    scene.pos[mid, 2] = np.linspace(4.0, 6.0, len(mid), dtype=np.float32)
    scene.opa[mid] = -2.5

    def pre(of):
        counts = np.bincount(of.ids, minlength=scene.n)
        assert (counts[big] > 256).all() and counts.max() <= 22 * 17
        assert (counts[mid] > 64).all() and (counts[mid] <= 256).all(), counts[mid]

    _run(gpu, scene, cam, f"workgroup-summed sh={use_sh} deg={deg}", 109, subset=(big + mid, 1e-4), precondition=pre)


# ------------------------------------------------------------------------------------------------------ 4. exp scales
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
def test_exp_scale_activation(gpu, use_sh, deg):
    """test_gpu_frame.py::test_frame_backward_exp_scale_activation with the maps: the depth term's chain under `exp`
    scales.  Tolerances exactly that test's (the activated scales differ by an ulp or two of expf before anything else
    happens): image 2e-4, rtol 1e-3, kappa 1e-4, l2 1e-3."""
    scene, cam = aux_case(5_000, 96, 80, seed=13, use_sh=use_sh, sh_degree=deg)
    scene.scale = np.log(np.abs(scene.scale) + 1e-4).astype(np.float32)
    of = OracleFrame(scene, cam, scale_activation="exp")
    gimg, gd, ga, n_masked = robust_aux_grads(of, 111)
    assert n_masked < SMALL_CAP * 96 * 80
    r, depth, alpha = _forward(gpu, of, scene, cam, dict(scale_activation="exp"), check=False)
    ref = of.aux_maps()
    g = of.grid
    dscale = max(1.0, float(np.abs(of.s_pos[:, 2]).max()))
    assert np.abs(r._keep[5].cpu().numpy() - of.image).max() < 2e-4
    assert np.abs(alpha.cpu().numpy() - g.crop(ref[:, :, 1:2])[:, :, 0]).max() < 2e-4
    assert np.abs(depth.cpu().numpy() - g.crop(ref[:, :, 0:1])[:, :, 0]).max() < 2e-4 * dscale
    _backward_three_ways(gpu, r, of, scene, gimg, gd, ga, f"exp scales sh={use_sh} deg={deg}",
                         tol=dict(rtol=1e-3, kappa=1e-4, l2=1e-3))


# ----------------------------------------------------------------------------------------------- 5. prob / dist lists
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("method,dist_thresh,n,W,H", [("dist", 0.5, 12_000, 250, 186), ("dist", 0.3, 12_000, 333, 201),
                                                      ("dist", 1.0, 12_000, 96, 80), ("prob", 0.5, 15_000, 250, 186)])
def test_tile_list_methods(gpu, method, dist_thresh, n, W, H, use_sh, deg):
    """The shapes of test_gpu_frame.py::test_frame_tile_culling_method_dist / _prob: the pair list equals the oracle's
    calc_tile_list (asserted in _forward), and in a "dist" frame the gradient rows are laid out over the discs' bounding
    squares, of which only the listed tiles hold a row -- the depth float's row walk has to skip the holes too."""
    scene, cam = aux_case(n, W, H, seed=29, use_sh=use_sh, sh_degree=deg)
    _run(gpu, scene, cam, f"{method} {dist_thresh} {W}x{H} sh={use_sh} deg={deg}", 113,
         of_kw=dict(tile_culling_method=method, dist_thresh=dist_thresh),
         r_kw=dict(tile_culling_method=method, tile_culling_dist_thresh=dist_thresh), grow=(method == "dist"))


# ------------------------------------------------------------------------------------------------ 6. block boundaries
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025])
@pytest.mark.parametrize("force_strips", [True, False])
def test_block_boundaries(gpu, n, force_strips):
    """Gaussian counts around the 64-lane wave and the 256-thread block, both binning variants, rgb, half translucent."""
    scene, cam = aux_case(n, 96, 80, seed=100 + n)
    scene.pos[:, 2] = np.abs(scene.pos[:, 2]) + 1.0  # in front of the camera: tiny scenes should not be all culled
    scene.opa -= np.float32(2.0)
    of, r = _run(gpu, scene, cam, f"n={n} strips={force_strips}", 115 + n, r_kw=dict(force_strips=force_strips))
    assert r.binning_variant() == ("strip" if force_strips else "table")
    assert np.array_equal(r.debug_views()["visible"].cpu().numpy(), of.mask.astype(bool))


# ------------------------------------------------------------------------------------------------------ 7. sort modes
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("sort_mode", [0, 1, "2t"])
def test_sort_modes(gpu, sort_mode, use_sh, deg):
    """The base scene behind the radix sorts (0, 1) and the table variant of the binning ("2t"): same list, same gradients."""
    scene, cam = aux_case(5000, 128, 96, seed=13, use_sh=use_sh, sh_degree=deg)
    kw = dict(sort_mode=2, table_bin=True) if sort_mode == "2t" else dict(sort_mode=sort_mode)
    _run(gpu, scene, cam, f"sort mode {sort_mode} sh={use_sh} deg={deg}", 117, r_kw=kw)


# ------------------------------------------------------------------------------------------------------------ 8. empty
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
def test_empty_frame(gpu, use_sh, deg):
    """Everything behind the camera: maps exactly zero, gradients exactly zero, every NaN of the destinations overwritten."""
    scene, cam = aux_case(500, 64, 64, use_sh=use_sh, sh_degree=deg)
    scene.pos[:, 2] = -5.0
    of = OracleFrame(scene, cam)
    assert len(of.ids) == 0 and int(of.mask.sum()) == 0
    r, depth, alpha = _forward(gpu, of, scene, cam, {}, check=False)
    assert float(r._keep[5].abs().max()) == 0.0 and float(depth.abs().max()) == 0.0 and float(alpha.abs().max()) == 0.0
    assert float(r._aux_keep[2].abs().max()) == 0.0
    rng = np.random.default_rng(3)
    gimg = rng.normal(size=(64, 64, 3)).astype(np.float32)
    gd, ga = (rng.normal(size=(64, 64)).astype(np.float32) for _ in range(2))
    for way in WAYS:
        gi, d, a = _way(way, gimg, gd, ga)
        out = tuple(torch.full_like(p, float("nan")) for p in r._keep[:5])
        r.backward(_t(gpu, gi), out=out, grad_depth=_t(gpu, d), grad_alpha=_t(gpu, a))
        for x in out:
            assert float(x.abs().max()) == 0.0 and bool(torch.isfinite(x).all()), way


# ------------------------------------------------------------------------------------------------ 9. the loss's own maps
@pytest.mark.parametrize("use_sh,deg", COLOURS, ids=COLOUR_IDS)
@pytest.mark.parametrize("mode", ["residual", "expected"])
@pytest.mark.parametrize("shift", [-4.0, -5.0])
def test_depth_loss_maps_end_to_end(gpu, shift, mode, use_sh, deg):
    """The gradient maps training really feeds: gs_train.DepthLoss on the kernel's OWN depth / alpha maps of the translucent
    base scene -- sparse (exact zeros at the 30 % unmeasured target pixels: 0, negative, inf, NaN), 1 / count, and in
    "expected" mode a hard edge at A = depth_alpha_min = 0.5 -- through gs_frame_backward, against aux_backward fed the
    FLOAT64 loss gradient evaluated on the ORACLE's maps (gs_testutil.depth_loss_f64).  The two sides see maps that differ
    by rounding, so the target keeps every measured pixel's residual at 5 - 15 % of the depth (no sign is undecidable),
    and no pixel may sit within 1e-5 of the alpha edge.  With opa -= 4 every pixel of the scene has A >= 0.5 (oracle: mean
    alpha 0.87); with opa -= 5 the edge runs through the frame (A >= 0.5 on 82 % of the pixels)."""
    from gs_train import DepthLoss

    alpha_min = 0.5
    scene, cam = aux_case(5000, 128, 96, seed=13, use_sh=use_sh, sh_degree=deg)
    scene.opa += np.float32(shift)
    of = OracleFrame(scene, cam)
    H, W = of.image.shape[:2]
    _, _, _, n_masked = robust_aux_grads(of, 119)
    assert n_masked == 0 and saturated_share(of) < 0.01
    maps = of.aux_maps()
    D = of.grid.crop(maps[:, :, 0:1])[:, :, 0].astype(np.float64)
    A = of.grid.crop(maps[:, :, 1:2])[:, :, 0].astype(np.float64)
    assert int((np.abs(A - alpha_min) < 1e-5).sum()) == 0  # (else the edge makes the two sides differ legitimately)
    assert (float((A >= alpha_min).mean()) < 0.9) == (shift == -5.0)  # -5: the edge runs through the frame
    rng = np.random.default_rng(121)
    off = rng.choice([-1.0, 1.0], (H, W)) * rng.uniform(0.05, 0.15, (H, W))
    z = np.where(A > 1e-3, D / np.maximum(A, 1e-3), 1.0) * (1.0 + off)
    z = z.astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.30
    kind = rng.integers(0, 4, (H, W))
    z[bad & (kind == 0)] = 0.0
    z[bad & (kind == 1)] = -z[bad & (kind == 1)]
    z[bad & (kind == 2)] = np.inf
    z[bad & (kind == 3)] = np.nan
    _, _, _, count, _, _ = depth_loss_f64(D, A, z, mode, alpha_min, 1.0)
    assert 0.05 * H * W < count < 0.8 * H * W
    scale = 1.0 / count
    gd64, ga64, loss64, _, r64, _ = depth_loss_f64(D, A, z, mode, alpha_min, scale)
    measured = r64 != 0
    with np.errstate(invalid="ignore"):
        size = np.maximum(np.abs(D), np.abs(A * z.astype(np.float64))) if mode == "residual" else np.abs(z.astype(np.float64))
        assert float((np.abs(r64[measured]) / size[measured]).min()) > 0.02  # no residual's sign is undecidable
    gd, ga = gd64.astype(np.float32), ga64.astype(np.float32)
    assert float((gd == 0).mean()) > 0.25  # sparse
    ref, rscale = of.aux_backward(None, gd, ga)

    r, depth, alpha = _forward(gpu, of, scene, cam, {})
    dl = DepthLoss(H, W, mode, alpha_min, gpu)
    tgd, tga = dl(depth.contiguous(), alpha.contiguous(), _t(gpu, z), scale)
    vals = dl.values.cpu().numpy()
    assert int(vals[1]) == count and abs(float(vals[0]) - loss64) <= 1e-4 * abs(loss64), (vals, count, loss64)
    assert torch.equal(tgd == 0, _t(gpu, gd) == 0) and torch.equal(tga == 0, _t(gpu, ga) == 0)  # the same support
    out = tuple(torch.full_like(p, float("nan")) for p in r._keep[:5])
    r.backward(None, out=out, grad_depth=tgd, grad_alpha=tga)
    got = [x.cpu().numpy() for x in out]
    rep = assert_grads_close(got, ref, rscale, f"depth loss {mode} shift={shift} sh={use_sh} deg={deg}")
    print(f"AUXBWD depth loss {mode} shift={shift} sh={use_sh} deg={deg}:", {k: (v[0], "%.2e" % v[2]) for k, v in rep.items()})
    culled = ~of.mask.astype(bool)
    for x in got:
        assert np.all(x[culled] == 0)


# --------------------------------------------------------------------------------------------------------- 10. full size
def _box_blur5(a):
    """5 x 5 box sum with zero padding (float64)."""
    p = np.pad(a, 2)
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), axis=0), axis=1)
    return c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]


def _rgbd_step_maps(of):
    """dL/dD, dL/dA of mean |D - A z| (float64) for the target z = the oracle's own expected depth D / A where A >= 0.5
    (elsewhere unmeasured: zero gradient), box-blurred 5 x 5 over the measured pixels and scaled by 1.02, so that the
    residual has both signs and is not identically zero: an RGB-D step's maps, not noise."""
    maps = of.aux_maps()
    D = of.grid.crop(maps[:, :, 0:1])[:, :, 0].astype(np.float64)
    A = of.grid.crop(maps[:, :, 1:2])[:, :, 0].astype(np.float64)
    valid = A >= 0.5
    z = _box_blur5(np.where(valid, D / np.where(valid, A, 1.0), 0.0)) / np.maximum(_box_blur5(valid.astype(np.float64)), 1.0)
    z = np.where(valid, 1.02 * z, np.nan)
    gd, ga, _, count, r, _ = depth_loss_f64(D, A, z, "residual", 0.5, 1.0 / max(int(valid.sum()), 1))
    return gd, ga, count, r


@pytest.mark.parametrize("cfg", ["cfg2", "trained"])
def test_aux_full_size_backward_matches_oracle(gpu, cfg):
    """Full size as RGB-D steps: test_gpu_frame.py::test_full_size_backward_matches_oracle's scene cfg2 (376,467 rgb
    Gaussians) and the trained-like scene (724,312 rgb Gaussians, 3.9 M pairs, lists to 5,361, 0.16 % of the pixels
    saturate).  dL/dimage is the L1 sign gradient, the maps' gradients those of mean |D - A z| (_rgbd_step_maps), all
    zeroed on the masked pixels (< 0.2 % of the frame).  All three gradients and the maps alone (at this size the image
    term dominates most elements and would hide a wrong depth term inside the tolerance of the sum): assert_grads_close
    at the defaults, and the relative error against the double-precision chain within CALIB_K (CALIB_K_MAX at the
    maximum) of the oracle's own fp32 arithmetic's (assert_error_no_worse_than)."""
    from gs_scene import CONFIGS

    if cfg == "trained":
        W, H, use_sh = 1920, 1080, False
        scene = make_trained_like_scene()
    else:
        n, W, H, use_sh = CONFIGS[cfg]
        scene = make_scene(n, W, H, seed=2023, use_sh=use_sh, sh_degree=2)
    cam = make_camera(W, H)
    of = OracleFrame(scene, cam)
    if cfg == "trained":
        assert scene.n == 724_312 and len(of.ids) > 3_900_000 and _lists(of).max() == 5361
        assert saturated_share(of) < 0.01  # (measured 0.16 % of the pixels: the translucent regime's own precondition)
    gimg = (np.sign(of.image - 0.5) / of.image.size).astype(np.float32)
    gimg, n_masked = of.robust_grad_image(gimg)
    assert n_masked < FULL_CAP * W * H, (n_masked, W * H)
    keep = of.robust_grad_image(np.ones(of.image.shape, np.float32))[0][:, :, 0]
    gd64, ga64, count, res = _rgbd_step_maps(of)
    assert count > 0.02 * W * H
    assert float((res > 0).sum()) > 0.01 * count and float((res < 0).sum()) > 0.01 * count  # both signs
    gd, ga = (gd64 * keep).astype(np.float32), (ga64 * keep).astype(np.float32)
    r, _, _ = _forward(gpu, of, scene, cam, {})
    print(f"AUXBWD {cfg}: pairs {len(of.ids)}, longest list {int(_lists(of).max())}, masked pixels {n_masked} "
          f"({100.0 * n_masked / (W * H):.3f} %), measured depth pixels {count}, saturated share {saturated_share(of):.3f}")
    rep = _backward_three_ways(gpu, r, of, scene, gimg, gd, ga, cfg, ways=("all", "maps"))
    for way in ("all", "maps"):
        got, ref, _ = rep[way]
        gi, d, a = _way(way, gimg, gd, ga)
        truth = of.aux_backward_f64(gi, d, a)
        names = NAMES if way == "all" else NAMES[:4]  # (the maps carry no colour gradient: nothing to take quantiles of)
        calib = assert_error_no_worse_than(got[:len(names)], truth, ref, f"{cfg} [{way}]")
        for name, (qh, qr) in calib.items():
            print(f"CALIB aux {cfg} [{way}] {name}: hip", ["%.2e" % v for v in qh], "reference arithmetic",
                  ["%.2e" % v for v in qr])
