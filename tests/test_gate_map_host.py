"""CPU tier of the gate carried into seeding and mapping (include/gs_abi.h: gs_track_gate_mask_workspace_bytes,
gs_track_gate_mask, gs_loss_l1_ssim_weighted; gs_train.GateMask / WeightedImageLoss / Trainer.add_view(weight=);
gs_slam.SlamOptions.gate_map / SlamFrame.gated): the symbols and their bindings, every refusal of both calls on fake pointers
in the header's order (each comes before anything is enqueued), the Python surface's refusals and field positions, and the
float64 reference of tests/gate_map_ref.py against oracle/train_ref.py and against finite differences.  No kernel is
launched."""
import os
import types

import numpy as np
import pytest

from oracle import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 48, 64
NAN, INF = float("nan"), float("inf")


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_track_gate_mask_workspace_bytes", "gs_track_gate_mask", "gs_loss_l1_ssim_weighted"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_track_gate_mask_workspace_bytes(", "int gs_track_gate_mask(", "int gs_loss_l1_ssim_weighted("):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    q = _lib.gs_track_gate_mask_workspace_bytes
    assert q(H, W) == _lib.gs_loss_track_gated_workspace_bytes(H, W) and q(H, W) % 256 == 0  # the gated loss's layout
    for bad in ((0, 64), (48, 0), (-1, 64), (48, -7)):
        assert q(*bad) == 0


# the arguments of gs_track_gate_mask, all valid
IMG, D, A, TI, TZ, RO, WO, VAL, RD, RC, WS = (FAKE + i * (1 << 24) for i in range(11))


def _mask_call(**kw):
    from gaussian import _lib

    a = dict(image=IMG, depth=D, alpha=A, timg=TI, trange=TZ, h=H, w=W, amin=0.5, kd=10.0, kc=0.0, fd=0.0, fc=0.0, couple=1,
             ro=RO, wo=WO, val=VAL, rd=RD, rc=RC, ws=WS, nbytes=_lib.gs_track_gate_mask_workspace_bytes(H, W))
    a.update(kw)
    return _lib.gs_track_gate_mask(a["image"], a["depth"], a["alpha"], a["timg"], a["trange"], a["h"], a["w"], a["amin"], a["kd"],
                                   a["kc"], a["fd"], a["fc"], a["couple"], a["ro"], a["wo"], a["val"], a["rd"], a["rc"], a["ws"],
                                   a["nbytes"], None)


def _mask_refused(word, **kw):
    from gaussian import _lib

    assert _mask_call(**kw) == GS_E_INVALID, kw
    msg = _lib.gs_last_error()
    assert b"gs_track_gate_mask" in msg and word in msg, (kw, msg)


def test_mask_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    for hw in ((0, W), (H, 0), (-1, W), (H, -3)):
        _mask_refused(b"empty", h=hw[0], w=hw[1])
    big = _lib.gs_track_gate_mask_workspace_bytes(4096, 4097)
    _mask_refused(b"2^24", h=4096, w=4097, nbytes=big)  # one row beyond 2^24 pixels
    _mask_refused(b"2^24", h=1, w=(1 << 24) + 1, nbytes=big)
    for kw in ("image", "depth", "alpha", "timg", "wo"):
        _mask_refused(b"null", **{kw: None})
    _mask_refused(b"both", trange=None)  # a range_out without a range ...
    _mask_refused(b"both", ro=None)      # ... and a range without a range_out
    for amin in (0.0, -0.5, NAN):
        _mask_refused(b"alpha_min", amin=amin)
    _mask_refused(b"NaN", kd=NAN)
    _mask_refused(b"NaN", kc=NAN)
    for bad in (-1.0, -1e-30, NAN):
        _mask_refused(b"floor", fd=bad)
        _mask_refused(b"floor", fc=bad)
    for kw, base in (("image", IMG), ("depth", D), ("alpha", A), ("timg", TI), ("trange", TZ), ("ro", RO), ("wo", WO),
                     ("rd", RD), ("rc", RC)):
        for off in (4, 8):
            _mask_refused(b"16-byte aligned", **{kw: base + off})  # the maps are walked float4 by float4
    _mask_refused(b"values_out", val=VAL + 2)
    n1 = 4 * H * W
    # an output inside an input, an input inside an output, an output on another output
    for kw in (dict(ro=TZ), dict(wo=TZ + n1 - 16), dict(ro=IMG + 3 * n1 - 16), dict(wo=A), dict(rd=D), dict(rc=TI + 16),
               dict(val=IMG + 4), dict(ro=A - n1 + 16)):
        _mask_refused(b"overlaps an input", **kw)
    for kw in (dict(wo=RO), dict(wo=RO + n1 - 16), dict(rd=RO), dict(rc=WO + 16), dict(val=WO + 4), dict(rd=RC)):
        _mask_refused(b"outputs overlap", **kw)
    _mask_refused(b"workspace", wo=RO + n1, ro=TZ + n1, ws=None)  # adjacent maps do not overlap: the next check speaks
    _mask_refused(b"workspace", ws=None)
    _mask_refused(b"workspace", ws=WS + 8)
    _mask_refused(b"workspace", nbytes=_lib.gs_track_gate_mask_workspace_bytes(H, W) - 1)
    _mask_refused(b"workspace", nbytes=0)
    # the RGB-only gate and the optional outputs pass every check (the call itself then needs a device: not made here)


def test_mask_refusals_come_in_the_headers_order():
    """Everything wrong at once; mending the first complaint each time walks through the header's list in its order."""
    bad = dict(h=0, image=None, trange=None, amin=0.0, kd=NAN, fd=-1.0, depth=D + 4, val=VAL + 2, wo=A, ws=None)
    order = [(b"empty", dict(h=1 << 13, w=(1 << 11) + 1)), (b"2^24", dict(h=H, w=W)), (b"null", dict(image=IMG)),
             (b"both", dict(trange=TZ)), (b"alpha_min", dict(amin=0.5)), (b"NaN", dict(kd=10.0)), (b"floor", dict(fd=0.0)),
             (b"16-byte aligned", dict(depth=D)), (b"values_out", dict(val=VAL)), (b"overlaps an input", dict(wo=WO)),
             (b"workspace", None)]
    for word, fix in order:
        _mask_refused(word, **bad)
        if fix is not None:
            bad.update(fix)  # mend the first complaint, keep the rest (the last one stays: no call is ever accepted)


P, T, M, G, LO, LWS = (FAKE + i * (1 << 24) for i in range(6))


def _loss_call(**kw):
    from gaussian import _lib

    a = dict(pred=P, target=T, weight=M, h=H, w=W, sw=0.1, s=float(H * W), si=float((H - 10) * (W - 10)), grad=G, out=LO, ws=LWS,
             nbytes=_lib.gs_loss_workspace_bytes(H, W))
    a.update(kw)
    return _lib.gs_loss_l1_ssim_weighted(a["pred"], a["target"], a["weight"], a["h"], a["w"], a["sw"], a["s"], a["si"], a["grad"],
                                         a["out"], a["ws"], a["nbytes"], None)


def _loss_refused(word, **kw):
    from gaussian import _lib

    assert _loss_call(**kw) == GS_E_INVALID, kw
    msg = _lib.gs_last_error()
    assert b"gs_loss_l1_ssim_weighted" in msg and word in msg, (kw, msg)


def test_weighted_loss_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    for hw in ((0, W), (H, 0), (-1, W), (H, -3)):
        _loss_refused(b"empty", h=hw[0], w=hw[1])
    for kw in ("pred", "target", "weight", "grad"):
        _loss_refused(b"null", **{kw: None})
    for sw in (-0.1, 1.5, NAN):
        _loss_refused(b"ssim_weight", sw=sw)
    for hw in ((10, W), (H, 10), (5, 7)):
        _loss_refused(b"window", h=hw[0], w=hw[1])
    for bad in (-1.0, NAN, INF, -INF):
        _loss_refused(b"weight_sum", s=bad)
        _loss_refused(b"weight_sum", si=bad)
    _loss_refused(b"workspace", ws=None)
    _loss_refused(b"workspace", nbytes=_lib.gs_loss_workspace_bytes(H, W) - 1)
    # in the header's order: everything wrong at once, mended one by one
    bad = dict(h=0, pred=None, sw=2.0, s=-1.0, ws=None)
    for word, fix in ((b"empty", "h"), (b"null", "pred"), (b"ssim_weight", "sw"), (b"weight_sum", "s"), (b"workspace", "ws")):
        _loss_refused(word, **bad)
        del bad[fix]
    bad = dict(h=8, sw=0.5, s=NAN)
    _loss_refused(b"window", **bad)


def test_python_surface_refusals_and_field_positions():
    import torch

    import gs_slam
    import gs_track
    import gs_train

    with pytest.raises(RuntimeError, match="no CPU fallback"):  # HIP kernels
        gs_train.GateMask(48, 64, 0.5, 10.0, 0.0, 0.0, 0.0, True, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs_train.GateMask.from_track_options(48, 64, gs_track.TrackOptions(depth_gate_k=10.0), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs_train.WeightedImageLoss(48, 64, 0.1, "cpu")
    # Trainer.add_view(weight=) validates before anything is appended: a Trainer's own state is not needed to be refused
    tr = object.__new__(gs_train.Trainer)
    tr.depths, tr.weights, tr._weight_sums, tr._depth_device, tr.cameras, tr.targets = None, None, None, "cpu", [], []
    cam = types.SimpleNamespace(height=12, width=16)
    img = torch.zeros(12, 16, 3)
    good = torch.ones(12, 16)
    neg, nan, inf = good.clone(), good.clone(), good.clone()
    neg[3, 4], nan[0, 0], inf[11, 15] = -1e-6, NAN, INF
    for bad, word in ((torch.ones(16, 12), "float32 .H,W."), (torch.ones(12, 16, 1), "float32 .H,W."),
                      (torch.ones(12, 16, dtype=torch.float64), "float32 .H,W."), (np.ones((12, 16), np.float32), "float32 .H,W."),
                      (neg, "not negative"), (nan, "finite"), (inf, "finite")):
        with pytest.raises(ValueError, match=word):
            tr.add_view(cam, img, None, weight=bad)
        assert tr.cameras == [] and tr.targets == [] and tr.weights is None
    assert tr.add_view(cam, img, None, weight=None) == 0 and tr.weights is None  # no map: the lists it always kept
    assert tr.add_view(cam, img, None, weight=good) == 1
    assert tr.weights[0] is None and torch.equal(tr.weights[1], good)
    assert tr._weight_sums == [(0.0, 0.0), (192.0, 12.0)]  # 12 x 16, interior 2 x 6: taken once, in double
    assert gs_train.weight_sums(torch.ones(10, 40)) == (400.0, 0.0)

    o = gs_slam.SlamOptions()
    assert o.gate_map is False
    names = list(gs_slam.SlamOptions.__dataclass_fields__)
    assert names[-2:] == ["gate_map", "icp"]  # in front of icp, which stays last
    fields = list(gs_slam.SlamFrame.__dataclass_fields__)
    assert fields[-2:] == ["gated", "icp"] and gs_slam.SlamFrame.__dataclass_fields__["gated"].default is None
    assert fields[:8] == ["rot", "tran", "tracked", "keyframe", "overlap", "window", "added", "map_losses"]
    f = gs_slam.SlamFrame(rot=np.eye(3), tran=np.zeros(3), tracked=None, keyframe=True, overlap=None)
    assert f.gated is None
    # gate_map needs a gated tracker: refused before any device work (no device is named, no camera field is read)
    for track in (gs_track.TrackOptions(), gs_track.TrackOptions(depth_gate=2.0)):
        with pytest.raises(ValueError, match="gate_map .* needs a gated tracker"):
            gs_slam.Slam(object(), gs_slam.SlamOptions(gate_map=True, track=track), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a gated tracker passes that check and meets the next
        gs_slam.Slam(types.SimpleNamespace(near=0.3), gs_slam.SlamOptions(gate_map=True, track=gs_track.TrackOptions(depth_gate_k=10.0)),
                     device="cpu")


# ---------------------------------------------------------------------------------------------------------------------
def _images(h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (h, w, 3))
    y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1)
    return x, y


@pytest.mark.parametrize("h,w,sw", [(13, 14, 0.3), (37, 53, 0.1), (12, 40, 1.0), (9, 20, 0.0)])
def test_reference_with_ones_is_the_unweighted_oracle(h, w, sw):
    from gate_map_ref import weighted_l1_ssim_loss

    x, y = _images(h, w, 7 * h + w)
    lo, l1, ssim, grad = train_ref.l1_ssim_loss(x, y, sw)
    wlo, wl1, wssim, wgrad = weighted_l1_ssim_loss(x, y, np.ones((h, w)), sw)
    assert abs(wlo - lo) <= 1e-12 and abs(wl1 - l1) <= 1e-12 and abs(wssim - ssim) <= 1e-12
    assert np.abs(wgrad - grad).max() <= 1e-12
    # a uniform scaling of the weights changes nothing: both terms are weighted means
    slo, sl1, sssim, sgrad = weighted_l1_ssim_loss(x, y, np.full((h, w), 0.37), sw)
    assert abs(slo - lo) <= 1e-12 and np.abs(sgrad - grad).max() <= 1e-12


def test_reference_gradient_against_finite_differences():
    """13 x 14, float weights with zeros: central differences of the helper's own loss, 1e-6 of the largest gradient entry.
    (|x - y| stays 0.02 away from the kink of the L1 term.)"""
    from gate_map_ref import weighted_l1_ssim_loss

    h, w, sw, eps = 13, 14, 0.3, 1e-5
    rng = np.random.default_rng(5)
    x = rng.uniform(0.1, 0.9, (h, w, 3))
    y = x + rng.choice([-1.0, 1.0], x.shape) * rng.uniform(0.02, 0.1, x.shape)
    m = rng.uniform(0, 1, (h, w))
    m[rng.uniform(size=(h, w)) < 0.2] = 0.0
    assert m[5:h - 5, 5:w - 5].sum() > 0
    _, _, _, grad = weighted_l1_ssim_loss(x, y, m, sw)
    fd = np.zeros_like(grad)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        fd[idx] = (weighted_l1_ssim_loss(xp, y, m, sw)[0] - weighted_l1_ssim_loss(xm, y, m, sw)[0]) / (2 * eps)
    err = np.abs(fd - grad).max() / np.abs(grad).max()
    print(f"weighted reference vs central differences: {err:.2e} of max |grad| = {np.abs(grad).max():.3e}")
    assert err <= 1e-6


def test_reference_zero_sums():
    from gate_map_ref import gate_mask_ref, weighted_l1_ssim_loss

    x, y = _images(13, 14, 3)
    assert weighted_l1_ssim_loss(x, y, np.zeros((13, 14)), 0.3)[:3] == (0.0, 0.0, 0.0)
    border = np.ones((13, 14))
    border[5:8, 5:9] = 0.0  # the whole interior
    lo, l1, ssim, grad = weighted_l1_ssim_loss(x, y, border, 0.3)
    assert ssim == 0.0 and lo == 0.7 * l1 and l1 > 0 and not grad[5:8, 5:9].any()
    # the mask contract with both gates off: the measured input, all ones
    from track_ref import ALPHA_MIN, loss_inputs, measured

    I, D, A, T, z = loss_inputs(7, 9, 16)
    rng, weight, values, _ = gate_mask_ref(I, D, A, T, z, ALPHA_MIN, 0.0, 0.0)
    assert np.array_equal(rng, np.where(measured(z), z, 0).astype(np.float32)) and np.all(weight == 1)
    assert values[0] == values[1] == measured(z).sum() and values[2] == 0 and values[3] == 63 and values[4] == 0
