"""GPU parity of the frame, cull and scene-pack paths on the whole raw scale domain.

gs_scene.make_scene only produces raw scales > 0 and the one exp case of the suite has no visible raw component above +1, so
every other frame-path test leaves three pieces of code unrun: the `sraw < 0` and `== 0` arms of the abs activation's backward
(frame_project_backward_body.inc, in every instantiation: plain, fused Adam, AUX, POSE), the upper end of the exp backward's
clamp to [-1, 1], and -- culled or packed -- phase A's own largest activated scale (gs_exp2 in cull_project.hip, expf through
make_static in the scene pack) under exp or on a negative raw scale.  An optimiser walks scales through zero, and seeding writes
exact zeros (seed_apply_body.inc).

This file runs the bodies of the existing tests -- check_forward (test_gpu_frame.py), _image_backward
(test_gpu_general_camera.py), _fused_pair / _assert_same (test_gpu_rgbd.py), check_pose_gradient (test_gpu_pose.py), the culled
and packed frame loop of test_gpu_scene_pack.py -- with their tolerances unchanged on inputs from gs_testutil.signed_raw_domain
and spread_exp_domain, each of which tests/test_raw_domain_host.py and tests/test_general_camera_host.py prove on the CPU to be
what it claims.  An oracle frame is computed once per case (gs_testutil.general_frame) and shared, read only.

Each comparison prints a line "RAWDOM ..." with the worst err / tol, or "bit-equal": profiles/raw_domain_parity.txt.
"""
import numpy as np
import pytest
import torch

from gs_frame import FrameRenderer
from gs_testutil import (GENERAL_CASES, GRAD_KAPPA, GRAD_RTOL, OracleFrame, assert_grads_close, general_case, general_frame,
                         raw_cull_camera, raw_cull_case, to_torch)
from test_gpu_frame import IMG_ATOL, check_forward
from test_gpu_general_camera import _image_backward, _worst
from test_gpu_pose import check_pose_gradient
from test_gpu_rgbd import _assert_same, _fused_pair
from test_gpu_scene_pack import _same_frame

pytestmark = pytest.mark.gpu

BACKWARD_KEYS = ["raw_signed_rgb", "raw_signed_sh2", "raw_exp_spread"]
# test_frame_backward_exp_scale_activation's arguments (expf differs by ulps before projection), for the exp case alone
EXP_TOL = dict(rtol=1e-3, kappa=1e-4, l2=1e-3)
EXP_IMG_ATOL = 2e-4


def _is_exp(key):
    return GENERAL_CASES[key]["exp"]


def _r_kw(key, **kw):
    return dict(kw, scale_activation="exp") if _is_exp(key) else kw


# -------------------------------------------------------------------------------------------------------------- a. forward
_EXP_FRAMES = {}


def _frame_behind_device_exp(gpu, key):
    """The oracle's frame of an exp case on the DEVICE's activated scales (OracleFrame's ``activated``: torch.exp on the GPU,
    the same library function the kernels call), computed once.  numpy.exp and the device's expf differ in the last bit on
    some of the ~11,000 visible components, and the projected covariances follow: bit equality of the records is a statement
    about the projection behind the activation, and that is what this frame isolates.  The pair list it gives must be
    general_frame's own, which every comparison with numpy.exp's frame (the backward below) rests on.  -> (frame, largest
    difference between the two activations in ulp)"""
    if key not in _EXP_FRAMES:
        scene, cam, of = general_frame(key)
        sn = torch.exp(torch.from_numpy(scene.scale).to(gpu)).cpu().numpy()
        ulp = float(np.abs(sn.view(np.int32).astype(np.int64) - of.sn.view(np.int32)).max())
        dev = OracleFrame(scene, cam, scale_activation="exp", activated=(of.qn, sn))
        assert np.array_equal(dev.keys, of.keys) and np.array_equal(dev.ids, of.ids) and np.array_equal(dev.accum, of.accum)
        assert np.array_equal(dev.mask, of.mask)
        _EXP_FRAMES[key] = (dev, ulp)
    return _EXP_FRAMES[key]


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("key", BACKWARD_KEYS)
def test_forward_parity(gpu, key, training):
    """Pair list, tile ranges and projected records bit for bit, image within IMG_ATOL (exp: 2e-4)."""
    scene, cam, of = general_frame(key)
    img_atol, note = IMG_ATOL, ""
    if _is_exp(key):
        img_atol = EXP_IMG_ATOL
        of, ulp = _frame_behind_device_exp(gpu, key)
        note = f" (oracle behind the device's exp, which differs from numpy.exp by at most {ulp:.0f} ulp; same pair list)"
    _, r, params = check_forward(gpu, scene, cam, training=training, of=of, img_atol=img_atol, r_kw=_r_kw(key))
    assert r._frame.scale_activation == int(_is_exp(key))
    image, _ = r.forward(*params, cam)
    print(f"RAWDOM forward {key} training={training}: pairs {len(of.ids)}, lists and records bit-equal{note}, image err/tol",
          round(float(np.abs(image.cpu().numpy() - of.image).max()) / img_atol, 3))


# ------------------------------------------------------------------------------------------------------------- b. backward
def _tolerance(ref, scale, rtol=GRAD_RTOL, kappa=GRAD_KAPPA, **_):
    """The element's own tolerance of gs_testutil.grad_close (without its floors: the larger of the two is the stricter test
    of "|ref| exceeds its tolerance")."""
    return rtol * np.abs(np.asarray(ref, np.float64)) + kappa * np.asarray(scale, np.float64)


def _backward_parity(gpu, key, what, **r_kw):
    """_image_backward with the case's tolerances, then what the shared helper cannot see.  -> its return value"""
    tol = EXP_TOL if _is_exp(key) else {}
    extra = dict(img_atol=EXP_IMG_ATOL) if _is_exp(key) else {}
    scene = general_frame(key)[0]
    of, r, grads, ref, scale = _image_backward(gpu, key, what, r_kw=_r_kw(key, **r_kw), **extra, **tol)
    assert r._frame.scale_activation == int(_is_exp(key))
    report = assert_grads_close(grads, ref, scale, f"raw domain {key}, {what}", **tol)
    print(f"RAWDOM backward {key} {what}: worst err/tol", _worst(report))
    vis = of.mask != 0
    s, got, want = scene.scale, grads[2], ref["scale"]
    if not _is_exp(key):
        zero = (s == 0) & vis[:, None]
        assert zero.sum() >= 100
        assert np.all(got.view(np.uint32)[zero] == 0), "scale gradient at a zero raw component is not +0.0"
        sure = (s < 0) & vis[:, None] & (np.abs(want) > _tolerance(want, scale["scale"]))
        assert sure.sum() >= 1_000, int(sure.sum())  # (tests/test_raw_domain_host.py: a condition on the input)
        assert np.array_equal(np.sign(got[sure]), np.sign(want[sure])), "sign of the scale gradient on negative raw scales"
        print(f"RAWDOM backward {key} {what}: scale gradient bit-equal to +0.0 at {int(zero.sum())} zero raw components, sign "
              f"equal to the oracle's on {int(sure.sum())} negative ones above their tolerance")
    else:
        above = np.nonzero((s > 1).any(axis=1) & vis)[0]
        assert len(above) >= 500, len(above)
        sub = assert_grads_close([g[above] for g in grads], {k: v[above] for k, v in ref.items()},
                                 {k: v[above] for k, v in scale.items()}, f"raw domain {key}, a raw scale above +1", **tol)
        print(f"RAWDOM backward {key} {what}: the {len(above)} Gaussians with a raw scale above +1, worst err/tol", _worst(sub))
    return of, r, grads, ref, scale


@pytest.mark.parametrize("key", BACKWARD_KEYS)
def test_backward_parity(gpu, key):
    _backward_parity(gpu, key, "pixel-parallel")


def test_backward_parity_row_layout(gpu):
    """raster_backward_rows_kernel (GS_FRAME_BWD_ROWS) in front of the same projection backward."""
    _, r, _, _, _ = _backward_parity(gpu, "raw_signed_rgb", "row layout", bwd_rows=True)
    assert r._frame.flags & 64


# ----------------------------------------------------------------------------------------------------------- c. fused step
@pytest.mark.parametrize("aux", [False, True])
def test_fused_backward_adam_equals_backward_then_adam(gpu, aux):
    """The sign select under ADAM != 0: parameters, both moments and the gradient statistic bit for bit."""
    scene, cam, _ = general_case("raw_signed_adam")
    _assert_same(_fused_pair(gpu, scene, cam, "max", True, 4, max_pairs=1 << 20, aux=aux), "max")
    print(f"RAWDOM fused backward + Adam raw_signed_adam aux={aux}: bit-equal to backward then Adam over 4 steps")


# -------------------------------------------------------------------------------------------------------- d. pose gradient
@pytest.mark.parametrize("aux", [False, True])
def test_pose_gradient_matches_fp64_oracle(gpu, aux):
    scene, cam, of = general_frame("raw_signed_pose")
    worst = check_pose_gradient(gpu, scene, cam, aux, of=of)
    print(f"RAWDOM pose gradient raw_signed_pose aux={aux}: worst err/tol", round(worst, 3))
    assert worst <= 1


# ----------------------------------------------------------------------------------------------- e. culled and packed frames
@pytest.mark.parametrize("scene_pack", [True, False], ids=["packed", "raw"])
@pytest.mark.parametrize("domain", ["signed", "exp"])
def test_culled_frames_are_bit_exact(gpu, domain, scene_pack):
    """Phase A's own largest activated scale (raw: fabsf / gs_exp2; packed: the pack's, from make_static) on negative and zero
    raw scales and under exp: six frames, three at rest and three after a 0.3 degree yaw; every image equals the unculled raw
    renderer's bit for bit, pairs and visible count equal the culled raw renderer's, and the cull emits fewer pairs."""
    scene, _, act = raw_cull_case(domain)
    params = to_torch(scene, gpu)
    kw = dict(scale_activation=act, force_strips=True, auto_grow=False, max_pairs=1 << 20)
    r = FrameRenderer(gpu, occlusion_cull=True, scene_pack=None if scene_pack else False, **kw)  # (None: automatic)
    cull_raw = FrameRenderer(gpu, occlusion_cull=True, scene_pack=False, **kw)
    off = FrameRenderer(gpu, occlusion_cull=False, scene_pack=False, **kw)
    r.CULL_MAX_SHIFT_PX = cull_raw.CULL_MAX_SHIFT_PX = float("inf")
    emitted = []
    for k, yaw in enumerate([0.0, 0.0, 0.0, 0.3, 0.3, 0.3]):
        cam = raw_cull_camera(domain, yaw)
        r._cull_off_until = cull_raw._cull_off_until = 0  # (the adaptive policy kept out of the way)
        ref, _ = off.forward(*params, cam)
        full = off.stats()
        img, _ = r.forward(*params, cam)
        st = r.stats()
        other, _ = cull_raw.forward(*params, cam)
        st_raw = cull_raw.stats()
        assert full.overflow == 0 and st.overflow == 0 and st_raw.overflow == 0, (k, st, st_raw)
        assert _same_frame(img, ref) and _same_frame(other, ref), (k, yaw, st, st_raw)
        assert bool(r._frame.flags & 256) == bool(cull_raw._frame.flags & 256) == (k >= 1), k
        assert r.scene_pack_active() == (scene_pack and k >= 1) and not cull_raw.scene_pack_active(), k
        assert (st.pairs, st.visible) == (st_raw.pairs, st_raw.visible), (k, st, st_raw)
        if k in (1, 2):  # static, no fallback: the cull must have culled, or this test hides a failure
            assert not st.cull_fallback and not st_raw.cull_fallback, (k, st, st_raw)
            assert st.pairs < full.pairs, (k, st, full)
        emitted.append(f"{st.pairs}/{full.pairs}" + ("f" if st.cull_fallback else ""))
    print(f"RAWDOM culled frames {domain} scene_pack={scene_pack}: 6 images bit-equal to the unculled raw renderer's, pairs and "
          f"visible equal to the culled raw renderer's; pairs emitted/unculled (f = fell back)", " ".join(emitted))

