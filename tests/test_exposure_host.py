"""CPU tier of the per-view exposure: the argument refusals of gs_exposure_apply / gs_exposure_backward through the C ABI (no
kernel is launched: every refusal comes before anything is enqueued), the option refusals of the Python layer, and the
restatement's own consistency (tests/exposure_ref.py).  The kernels meet the restatement in tests/test_gpu_exposure.py."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import exposure_ref as X

GS_E_INVALID = -1


def _aligned(nbytes, align=256):
    """A host buffer whose address is a multiple of ``align``: (keep-alive object, address).  Never dereferenced."""
    raw = C.create_string_buffer(nbytes + align)
    return raw, (C.addressof(raw) + align - 1) // align * align


def test_abi_refusals_without_a_gpu():
    from gaussian import _lib

    H, W = 5, 7
    nbytes = H * W * 12
    (k1, img), (k2, out), (k3, num), (k4, ws), (k5, st) = (_aligned(nbytes), _aligned(nbytes), _aligned(24), _aligned(4096),
                                                            _aligned(128))
    need = _lib.gs_exposure_workspace_bytes(H, W)
    assert need == 256 and _lib.gs_exposure_workspace_bytes(1080, 1920) == 48 * 2025 + (-48 * 2025) % 256
    assert _lib.gs_exposure_workspace_bytes(0, 7) == 0 and _lib.gs_exposure_workspace_bytes(5, -1) == 0
    assert C.sizeof(_lib.GsExposureState) == 104
    ap = _lib.gs_exposure_apply
    for args, word in (((None, num, H, W, out, None), b"null"), ((img, None, H, W, out, None), b"null"),
                       ((img, num, H, W, None, None), b"null"), ((img, num, 0, W, out, None), b"empty"),
                       ((img, num, H, -3, out, None), b"empty"), ((img + 4, num, H, W, out, None), b"16-byte"),
                       ((img, num, H, W, out + 8, None), b"16-byte"), ((img, num + 2, H, W, out, None), b"4-byte"),
                       ((img, num, H, W, img, None), b"alias"), ((img, num, H, W, img + 16, None), b"alias")):
        assert ap(*args) == GS_E_INVALID, args
        assert word in _lib.gs_last_error(), (word, _lib.gs_last_error())
    bw = _lib.gs_exposure_backward

    def adam(**kw):
        d = dict(state=st, lr_gain=1e-2, lr_bias=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lr_scale=1.0, skip_if_nonzero=None)
        d.update(kw)
        return C.byref(_lib.GsExposureAdam(**d))

    nan = float("nan")
    cases = [((None, out, num, H, W, None, None, ws, need, None), b"null"),
             ((img, None, num, H, W, None, None, ws, need, None), b"null"),
             ((img, out, None, H, W, None, None, ws, need, None), b"null"),
             ((img, out, num, 0, W, None, None, ws, need, None), b"empty"),
             ((img, out, num, H, 0, None, None, ws, need, None), b"empty"),
             ((img + 8, out, num, H, W, None, None, ws, need, None), b"16-byte"),
             ((img, out + 4, num, H, W, None, None, ws, need, None), b"16-byte"),
             ((img, out, num + 1, H, W, None, None, ws, need, None), b"4-byte"),
             ((img, out, num, H, W, num + 2, None, ws, need, None), b"4-byte"),
             ((img, img, num, H, W, None, None, ws, need, None), b"alias"),
             ((img, out, num, H, W, num, None, None, need, None), b"workspace"),
             ((img, out, num, H, W, num, None, ws, need - 1, None), b"workspace"),
             ((img, out, num, H, W, num, None, ws + 4, need, None), b"workspace"),
             ((img, out, num, H, W, None, adam(state=None), ws, need, None), b"state"),
             ((img, out, num, H, W, None, adam(state=st + 4), ws, need, None), b"8-byte"),
             ((img, out, num, H, W, None, adam(skip_if_nonzero=st + 4), ws, need, None), b"8-byte")]
    for key in ("lr_gain", "lr_bias", "lr_scale"):
        for bad in (-1e-3, nan, math.inf):
            cases.append(((img, out, num, H, W, None, adam(**{key: bad}), ws, need, None), b"lr_"))
    for bad in (-1e-8, nan):
        cases.append(((img, out, num, H, W, None, adam(eps=bad), ws, need, None), b"eps"))
    for key in ("beta1", "beta2"):
        for bad in (-0.1, nan, 1.0):
            cases.append(((img, out, num, H, W, None, adam(**{key: bad}), ws, need, None), b"betas"))
    for args, word in cases:
        assert bw(*args) == GS_E_INVALID, args
        assert word in _lib.gs_last_error(), (word, _lib.gs_last_error())
    del k1, k2, k3, k4, k5


def test_python_refusals_need_no_device():
    import gs_exposure
    import gs_slam
    import gs_track
    import gs_train

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs_exposure.Exposure(12, 16, "cpu")
    for bad in (dict(gain=(1, 1)), dict(bias=(0, 0, 0, 0)), dict(gain=(1, float("nan"), 1)), dict(bias=(0, math.inf, 0))):
        with pytest.raises(ValueError):
            gs_exposure.numbers32(**bad)
    assert gs_exposure.numbers32().tolist() == [1, 1, 1, 0, 0, 0] and gs_exposure.numbers32().dtype == np.float32
    # the options: off by default, the rates those of the exposure-only fit
    o = gs_track.TrackOptions()
    assert o.fit_exposure is False and o.fits_exposure() is False and o.lr_gain == 3e-2 and o.lr_bias == 3e-2
    assert gs_track.TrackResult(np.eye(3), np.zeros(3), 0.0, 0).exposure is None
    s = gs_slam.SlamOptions()
    assert s.refine_exposure is False and s.track.fit_exposure is False
    assert gs_slam.SlamFrame(rot=np.eye(3), tran=np.zeros(3), tracked=None, keyframe=True, overlap=None).exposure is None
    # fit_exposure with device_pose: refused by the options, by the Tracker and by Slam before any device work
    both = gs_track.TrackOptions(fit_exposure=True, device_pose=True)
    with pytest.raises(ValueError, match="fit_exposure is not available with device_pose"):
        both.fits_exposure()
    z = lambda *s_: torch.zeros(*s_)  # noqa: E731
    cam = types.SimpleNamespace(height=12, width=16, near=0.3)
    with pytest.raises(ValueError, match="fit_exposure is not available with device_pose"):
        gs_track.Tracker((z(10, 3), z(10, 4), z(10, 3), z(10), z(10, 3)), cam, both, device="cpu")
    with pytest.raises(ValueError, match="fit_exposure is not available with device_pose"):
        gs_slam.Slam(cam, gs_slam.SlamOptions(track=both), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # fit_exposure alone passes that check and meets the next
        gs_slam.Slam(cam, gs_slam.SlamOptions(track=gs_track.TrackOptions(fit_exposure=True)), device="cpu")
    # a free exposure under several ranks: refused before the view or the device is looked at
    tr = object.__new__(gs_train.Trainer)
    tr.world_size = 2
    with pytest.raises(RuntimeError, match="view parallelism"):
        tr.free_exposure(0, 1e-3, 1e-3)
    tr.world_size, tr.cameras, tr._exposure = 1, [cam], {}
    with pytest.raises(IndexError):
        tr.free_exposure(1, 1e-3, 1e-3)
    assert tr.exposure(0) is None  # a view without an exposure: no object, no read
    tr.fix_exposure(0)
    # keyframe 0 is the gauge: Slam never frees it
    sl = object.__new__(gs_slam.Slam)
    sl.opt, sl.trainer = gs_slam.SlamOptions(), None
    with pytest.raises(ValueError, match="keyframe 0 fixes the radiometric gauge"):
        sl.free_exposures([2, 0])
    sl.free_exposures([])


def test_restatement_identity_and_consistency():
    rng = np.random.default_rng(5)
    img = rng.random((31, 33, 3), dtype=np.float32)
    grad = rng.normal(size=(31, 33, 3)).astype(np.float32)
    grad[rng.random(grad.shape) < 0.2] = 0.0
    ident = X.numbers()
    assert X.apply(img, ident).tobytes() == img.tobytes()
    g, sums, bound = X.backward(img, grad, ident)
    assert g.tobytes() == grad.tobytes()
    # the sums against plain float64 sums in another order, inside the bound they state
    plain = np.concatenate([(grad.astype(np.float64) * img).sum(axis=(0, 1)), grad.astype(np.float64).sum(axis=(0, 1))])
    assert (np.abs(plain - sums) <= bound).all() and (bound < 1e-6 * np.abs(sums).max()).all()
    # two roundings, no contraction: against the products rounded by hand
    num = X.numbers(X.GAIN_STAR, X.BIAS_STAR)
    out = X.apply(img, num)
    for (y, x, c) in ((0, 0, 0), (17, 5, 1), (30, 32, 2)):
        want = X.f32(X.f32(float(num[c]) * float(img[y, x, c])) + float(num[3 + c]))
        assert float(out[y, x, c]) == want
    # the chain rule the kernels implement, against central differences of a linear functional of I' (exact in float64)
    lin = float((grad.astype(np.float64) * X.apply(img, num).astype(np.float64)).sum())
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-3
        up = (img.astype(np.float64) * (num[0:3] + e[0:3]) + (num[3:6] + e[3:6])) * grad
        dn = (img.astype(np.float64) * (num[0:3] - e[0:3]) + (num[3:6] - e[3:6])) * grad
        assert abs((up.sum() - dn.sum()) / 2e-3 - sums[k]) <= 1e-6 * max(1.0, abs(sums[k])), (k, lin)
    # Adam: the first step moves every number with a non-zero gradient by lr (bias corrections cancel), a zero gradient and
    # a raised skip flag move nothing, and the state counts
    st = X.new_state()
    g6 = [0.3, -2.0, 0.0, 1e-4, -1e-4, 5.0]
    new = X.step(st, ident, g6, X.default_opts(lr_gain=1e-2, lr_bias=1e-3))
    for k, (p, q) in enumerate(zip(ident.tolist(), new)):
        lr = 1e-2 if k < 3 else 1e-3
        want = p - lr * g6[k] / (abs(g6[k]) + 1e-8)  # (m / bc1 = g and sqrt(v / bc2) = |g| at the first step)
        assert abs(q - want) <= 1e-6 * lr + 2.0 ** -24, (k, q, want)
        assert q == X.f32(q)
    assert st["steps"] == 1.0
    frozen = {k: list(v) if isinstance(v, list) else v for k, v in st.items()}
    assert X.step(st, new, g6, X.default_opts(), skip=True) == new and st == frozen
    assert X.step(st, new, [float("nan")] + g6[1:], X.default_opts()) == new and st == frozen
    assert X.step(st, new, g6, X.default_opts(lr_gain=0.0, lr_bias=0.0)) == new and st["steps"] == 2.0
    s = X.tenth_scales()
    assert np.allclose(s, [0.3, 0.2, 0.1, 0.05, 0.03, 0.03])
