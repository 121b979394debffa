"""The inputs of tests/test_gpu_raw_domain.py are what they claim, proven on the oracle alone.

gs_scene.make_scene only produces raw scales > 0, and the one exp case derived from it (bwd_exp) has no visible raw component
above +1: the `sraw < 0` and `== 0` arms of the abs activation's backward and the upper end of the exp backward's clamp to
[-1, 1] are outside every other test's inputs.  gs_testutil.signed_raw_domain and spread_exp_domain put cases there; what is
asserted below are conditions on those INPUTS -- signs, zeros, clamp regimes, the oracle's own gradient on them, how much of
the cull scene saturates -- not measurements of code under test, and the figures the cases were chosen on, pinned exactly so
that a change of a generator is seen.  (That each case is a valid frame under general_camera -- visible share, list lengths,
masked pixels -- is tests/test_general_camera_host.py, which takes the keys from GENERAL_CASES.)"""
import numpy as np
import pytest

from gs_scene import Scene
from gs_testutil import GENERAL_CASES, GRAD_KAPPA, GRAD_RTOL, OracleFrame, general_frame, raw_cull_case, robust_aux_grads

SIGNED_KEYS = ["raw_signed_rgb", "raw_signed_sh2", "raw_signed_adam", "raw_signed_pose"]
SCALE_GRAD_KEYS = SIGNED_KEYS[:3]  # forward + backward against the oracle, fused step: the scale gradient is compared
ORACLE_BACKWARD_KEYS = SIGNED_KEYS[:2]  # compared with OracleFrame.backward element by element
GRAD_SEED = 4  # test_gpu_general_camera._image_backward's default: the dL/dimage the GPU comparison runs on


def visible_components(scene, of):
    """The raw scale components of the visible Gaussians, flat."""
    return scene.scale[of.mask != 0].ravel()


def exp_regimes(s):
    """-> (#components below -1, inside [-1, 1], above +1): the three regimes of the exp backward g exp(clamp(s, -1, 1))."""
    return int((s < -1).sum()), int(((s >= -1) & (s <= 1)).sum()), int((s > 1).sum())


def saturated_tiles(of):
    """-> (mask [tiles_y, tiles_x] of the 16 x 16 tiles whose every pixel stopped inside its list (oracle alpha > 0.9999),
    pairs per tile in the same shape)"""
    g = of.grid
    a = of.aux_maps()[:, :, 1]
    full = a.reshape(g.padded_height // 16, 16, g.padded_width // 16, 16).min(axis=(1, 3)) > 0.9999
    return full, np.diff(of.accum).reshape(full.shape)


def _robust_gimg(of):
    gimg = np.random.default_rng(GRAD_SEED).normal(size=of.image.shape).astype(np.float32)
    return of.robust_grad_image(gimg)[0]


@pytest.mark.parametrize("key", SIGNED_KEYS)
def test_signed_case_covers_both_signs_and_both_zeros(key):
    assert GENERAL_CASES[key]["signed"] and not GENERAL_CASES[key]["exp"]
    scene, cam, of = general_frame(key)
    s = visible_components(scene, of)
    zero = s == 0
    line = (f"raw domain case {key}: {int((s < 0).sum())} negative, {int((s > 0).sum())} positive, {int(zero.sum())} zero "
            f"({int((zero & np.signbit(s)).sum())} of them -0.0) of {s.size} visible raw components")
    assert (s < 0).mean() >= 0.3 and (s > 0).mean() >= 0.3, line
    assert (zero & ~np.signbit(s)).sum() >= 50 and (zero & np.signbit(s)).sum() >= 50, line
    nq = np.linalg.norm(scene.quat.astype(np.float64), axis=1)
    assert nq.min() < 1e-2 and nq.max() > 1e2, (nq.min(), nq.max())  # the raw quaternions are far from normalised
    print(line)


@pytest.mark.parametrize("key", SIGNED_KEYS)
def test_signed_case_oracle_gradient_sees_the_sign(key):
    """The oracle on the signed case: exactly 0 at every zero component, a nonzero gradient on the negative ones, and there
    minus the gradient of the frame with |scale| in place of scale -- which has the same activated values, so is the same
    frame: what the negative components add to a test is the sign select and nothing else.
    "Nonzero on at least 90 %" is taken over the negative components of the Gaussians that have a pair: the frustum test's
    margin is wider than the image, and the visible Gaussians beside it touch no tile and have no gradient whatever their
    sign.  Measured: raw_signed_rgb / _sh2 0.9024 (0.8554 of all visible negative components), raw_signed_adam 0.9622 (0.8976),
    raw_signed_pose 0.8784 (0.8267) -- the rest are listed behind the pixel's stop in every tile they touch.  The bound is
    asserted on the cases whose GPU comparison READS the scale gradient (SCALE_GRAD_KEYS); raw_signed_pose's compares the
    pose gradient alone, which passes through the activation and not through its backward's sign select: its share is
    printed, every other condition holds for it as for the others."""
    scene, cam, of = general_frame(key)
    gimg = _robust_gimg(of)
    ref = of.backward(gimg)
    assert all(np.isfinite(v).all() for v in ref.values())
    vis = of.mask != 0
    s, g = scene.scale[vis], ref["scale"][vis]
    assert np.all(g[s == 0] == 0.0), "the oracle's scale gradient is not zero at a zero raw component"
    neg = s < 0
    paired = np.zeros(scene.n, bool)
    paired[of.ids] = True
    listed = neg & paired[vis][:, None]
    nonzero = float((g[listed] != 0).mean())
    line = (f"raw domain case {key}: oracle scale gradient nonzero on {nonzero:.4f} of the {int(listed.sum())} negative "
            f"components of Gaussians with a pair ({float((g[neg] != 0).mean()):.4f} of all {int(neg.sum())} visible negative "
            f"ones), median |g| over the latter {float(np.median(np.abs(g[neg]))):.3e}")
    if key in SCALE_GRAD_KEYS:
        assert nonzero >= 0.9, line
    flipped = Scene(scene.pos, scene.quat, np.abs(scene.scale), scene.opa, scene.rgb)
    of_abs = OracleFrame(flipped, cam)
    assert np.array_equal(of_abs.sn.view(np.uint32), of.sn.view(np.uint32)) and np.array_equal(of_abs.ids, of.ids)
    assert np.array_equal(of_abs.padded.view(np.uint32), of.padded.view(np.uint32))
    ref_abs = of_abs.backward(gimg)
    g_abs = ref_abs["scale"][vis]
    assert np.array_equal(g[neg], -g_abs[neg]) and np.array_equal(g[s > 0], g_abs[s > 0])
    for name in ("pos", "quat", "opa", "rgb"):
        assert np.array_equal(ref[name], ref_abs[name]), name
    if key in ORACLE_BACKWARD_KEYS:
        # the GPU comparison asserts the gradient's SIGN where |ref| exceeds the element's own tolerance (grad_close's
        # rtol |ref| + kappa scale): not a vacuous statement -- measured 2,173 (rgb) and 2,168 (sh2) of the 5,359
        _, scale = of.backward(gimg, with_scale=True)
        sure = neg & (np.abs(g) > GRAD_RTOL * np.abs(g) + GRAD_KAPPA * scale["scale"][vis])
        assert sure.sum() >= 1_000, int(sure.sum())
    print(line)


def test_exp_spread_case_covers_both_ends_of_the_clamp():
    c = GENERAL_CASES["raw_exp_spread"]
    assert c["exp"] and c["spread"] == 8.0 and not c["signed"]
    scene, cam, of = general_frame("raw_exp_spread")
    assert of.scale_activation == "exp"
    below, inside, above = exp_regimes(visible_components(scene, of))
    n = below + inside + above
    line = f"raw domain case raw_exp_spread: {below} below -1, {inside} inside [-1, 1], {above} above +1 of {n}"
    assert min(below, inside, above) >= 0.15 * n, line
    print(line)


@pytest.mark.parametrize("domain", ["signed", "exp"])
def test_cull_scene_saturates_at_least_half_of_its_tiles(domain):
    """The occlusion cull has something to cull (the GPU test asserts fewer emitted pairs than the unculled frame): at least
    half the tiles saturate in every pixel."""
    scene, cam, act = raw_cull_case(domain)
    assert not cam.tran.any()  # (make_camera's translation is zero: scaling it by k leaves the camera where it was)
    of = OracleFrame(scene, cam, scale_activation=act)
    full, lens = saturated_tiles(of)
    line = (f"raw domain cull scene {domain}: {int(full.sum())} of {full.size} tiles saturate in every pixel, holding "
            f"{int(lens[full].sum())} of {len(of.ids)} pairs")
    assert full.sum() >= 0.5 * full.size, line
    s = visible_components(scene, of)
    if domain == "signed":
        assert (s < 0).mean() >= 0.3 and (s > 0).mean() >= 0.3 and (s == 0).sum() >= 100, line
    else:
        assert min(exp_regimes(s)) >= 0.15 * s.size, (line, exp_regimes(s))
    print(line)


def test_raw_domain_figures():
    """The figures the cases were chosen on, exactly (visible share to four places)."""
    def frame_figures(key):
        scene, cam, of = general_frame(key)
        return (round(float(of.mask.mean()), 4), len(of.ids), int(np.diff(of.accum).max()), robust_aux_grads(of, 1)[3],
                visible_components(scene, of))

    for key in ("raw_signed_rgb", "raw_signed_sh2"):
        vis, pairs, longest, masked, s = frame_figures(key)
        assert (vis, pairs, longest, masked) == (0.7258, 11_997, 423, 12), key
        zero = s == 0
        assert (int((s < 0).sum()), int((s > 0).sum()), int(zero.sum()), int((zero & np.signbit(s)).sum())) == \
            (5_359, 5_324, 204, 105), key
    vis, pairs, longest, masked, s = frame_figures("raw_exp_spread")
    assert (vis, pairs, longest, masked) == (0.7488, 12_109, 684, 12)
    assert exp_regimes(s) == (2_810, 6_146, 2_276)
    for domain, tiles, pairs_in, pairs, regimes in (("signed", 124, 51_047, 79_154, None),
                                                    ("exp", 134, 58_341, 82_708, (4_741, 6_492, 3_338))):
        scene, cam, act = raw_cull_case(domain)
        of = OracleFrame(scene, cam, scale_activation=act)
        full, lens = saturated_tiles(of)
        assert (full.size, int(full.sum()), int(lens[full].sum()), len(of.ids)) == (192, tiles, pairs_in, pairs), domain
        if regimes:
            assert exp_regimes(visible_components(scene, of)) == regimes
