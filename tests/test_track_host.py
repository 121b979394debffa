"""CPU tier of camera tracking (include/gs_abi.h: gs_loss_track_workspace_bytes, gs_loss_track; gs_train.TrackLoss;
gs_track.Tracker): the symbols and their ctypes bindings, the workspace size query, every refusal on fake pointers (each comes
before anything is enqueued), the Python surface's refusals and defaults, the rotation gradient of the pose step against a
finite difference, the constant-velocity prediction, the fp64 reference's own undecidable share for the seeds the GPU tier
uses, and the resources of the two kernels read from the built code object.  No kernel is launched."""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 48, 64


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_loss_track_workspace_bytes", "gs_loss_track"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_loss_track_workspace_bytes(", "int gs_loss_track("):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays
    assert "#define GS_ABI_VERSION 8" in header


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_loss_track_workspace_bytes
    sizes = [(1, 1), (7, 9), (48, 64), (187, 250), (480, 640), (1080, 1920), (2160, 3840)]
    got = [q(h, w) for h, w in sizes]
    for b in got:
        assert b > 0 and b % 256 == 0
    assert got == sorted(got) and got[-1] > got[0]  # monotone in H * W
    assert q(64, 48) == q(48, 64)
    # one 16-byte row per 1,024 pixels
    assert 16 * math.ceil(1080 * 1920 / 1024) <= got[5] < 16 * math.ceil(1080 * 1920 / 1024) + 256
    for bad in ((0, 64), (48, 0), (-1, 64), (48, -7), (0, 0)):
        assert q(*bad) == 0


def test_loss_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_loss_track_workspace_bytes(H, W)
    IMG, D, A, TI, TZ, GI, GD, GA, VAL, WS = (FAKE + i * (1 << 24) for i in range(10))

    def call(image=IMG, depth=D, alpha=A, timg=TI, trange=TZ, h=H, w=W, amin=0.5, cw=1.0, dw=1.0, gate=0.0, scale=1.0, gi=GI,
             gd=GD, ga=GA, val=VAL, ws=WS, nbytes=ws_bytes):
        return _lib.gs_loss_track(image, depth, alpha, timg, trange, h, w, amin, cw, dw, gate, scale, gi, gd, ga, val, ws,
                                  nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_loss_track" in msg and word in msg, (kw, msg)

    for kw in ("image", "depth", "alpha", "timg", "gi", "gd", "ga"):
        refused(b"null", **{kw: None})
    for hw in ((0, W), (H, 0), (-1, W), (H, -3)):
        refused(b"empty", h=hw[0], w=hw[1])
    for kw, base in (("image", IMG), ("depth", D), ("alpha", A), ("timg", TI), ("trange", TZ), ("gi", GI), ("gd", GD),
                     ("ga", GA)):
        for off in (4, 8):
            refused(b"16-byte aligned", **{kw: base + off})  # the maps are walked float4 by float4
    for amin in (0.0, -0.5, float("nan")):
        refused(b"alpha_min", amin=amin)
    for bad in (-1.0, -1e-30, float("nan")):
        refused(b"weight", cw=bad)
        refused(b"weight", dw=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"scale", scale=bad)
    refused(b"workspace", ws=None)
    refused(b"workspace", ws=WS + 8)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"values_out", val=VAL + 2)


def test_python_surface_refusals_and_defaults():
    import torch

    import gs_track
    import gs_train
    from gs_scene import make_camera

    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a HIP kernel
        gs_train.TrackLoss(48, 64, 0.5, 1.0, 1.0, 0.0, "cpu")
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    cam = make_camera(64, 48)
    for cd in (27, 48):
        with pytest.raises(RuntimeError, match="pose gradients need rgb colours: with SH colours the image also depends on "
                                               "the pose through each pixel's ray direction"):
            gs_track.Tracker((z(10, 3), z(10, 4), z(10, 3), z(10), z(10, cd)), cam, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # an rgb map gets as far as the device
        gs_track.Tracker((z(10, 3), z(10, 4), z(10, 3), z(10), z(10, 3)), cam, device="cpu")
    o = gs_track.TrackOptions()
    # tests/test_gpu_pose.py::test_pose_recovery: lr 2e-3 for both groups, down to 0.01 x over 300 iterations, alpha 0.5
    assert (o.iterations, o.lr_rot, o.lr_tran, o.lr_final, o.alpha_min) == (300, 2e-3, 2e-3, 0.01, 0.5)
    assert o.depth_gate <= 0.0  # off
    assert o.color_weight > 0 and o.depth_weight > 0
    assert [f for f in gs_track.TrackResult.__dataclass_fields__] == ["rot", "tran", "loss", "iterations", "losses"]


def test_rotation_gradient_matches_a_finite_difference():
    """dL/dw of rot(w) = exp([w]x) R at w = 0 for L = <G, rot>, G random: the formula of the pose step against a central
    difference in float64 through the power series of exp."""
    from gs_track import rot_tangent_grad, so3_exp
    from track_ref import so3_exp_series

    rng = np.random.default_rng(5)
    for _ in range(5):
        G = rng.normal(size=(3, 3))
        R = so3_exp_series(rng.normal(size=3))
        got = rot_tangent_grad(G, R)
        h = 1e-5
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd = (np.sum(G * (so3_exp_series(e) @ R)) - np.sum(G * (so3_exp_series(-e) @ R))) / (2 * h)
            assert abs(got[k] - fd) <= 1e-8 * np.abs(G).sum(), (k, got[k], fd)  # (truncation h^2 / 6 |G| ~ 2e-11 |G|)
    for w in (np.zeros(3), np.array([1e-10, 0, 0]), np.array([1e-3, -2e-3, 5e-4]), rng.normal(size=3), np.array([3.0, 0.5, -1.0])):
        E = so3_exp(w)
        assert np.abs(E - so3_exp_series(w, 60)).max() <= 1e-14
        assert np.abs(E @ E.T - np.eye(3)).max() <= 1e-14


def test_constant_velocity_prediction_reproduces_a_constant_twist():
    """T_k = Delta^k T_0: the prediction from T_1 and T_2 is T_3."""
    from gs_track import predict_constant_velocity
    from track_ref import so3_exp_series

    rng = np.random.default_rng(9)
    dR, dt = so3_exp_series(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.1
    R, t = so3_exp_series(rng.normal(size=3)), rng.normal(size=3)
    poses = [(R, t)]
    for _ in range(3):
        R, t = dR @ R, dR @ t + dt
        poses.append((R, t))
    Rp, tp = predict_constant_velocity(poses[1], poses[2])
    assert np.abs(Rp - poses[3][0]).max() <= 1e-14 and np.abs(tp - poses[3][1]).max() <= 1e-14
    assert np.abs(Rp @ Rp.T - np.eye(3)).max() <= 1e-14


def test_reference_and_restatement_on_the_gpu_tiers_inputs():
    """What tests/test_gpu_track.py relies on, from the fp64 reference alone: for its sizes and seeds the share of pixels
    whose sign of r or gate decision fp32 cannot be asked to reproduce is under the 0.1 % cap, the gate cuts roughly a tenth
    of the measured pixels inside the silhouette, the silhouette and the measurements split the image, some image entries
    equal their target exactly -- and the float32 restatement of the colour gradient is the fp64 one rounded."""
    from track_ref import ALPHA_MIN, GATE, LOSS_CASES, colour_grad_f32, loss_inputs, measured, track_loss_f64

    for Hh, Ww, seed in LOSS_CASES:
        I, D, A, T, z = loss_inputs(Hh, Ww, seed)
        n = Hh * Ww
        scale = 0.37 / n
        ref = track_loss_f64(I, D, A, T, z, ALPHA_MIN, 0.8, 1.3, GATE, scale)
        assert float(ref["undecidable"].sum()) / n <= 1e-3, (Hh, Ww)
        inside = ref["cmask"] & measured(z)
        if n > 1000:
            assert 0.05 < 1.0 - ref["count"] / inside.sum() < 0.2
            assert 0.3 < ref["cmask"].mean() < 0.7 and 0.6 < measured(z).mean() < 0.8
            assert 0.05 < (I == T).mean() < 0.15
        assert np.all(ref["grad_depth"][~ref["dmask"]] == 0) and np.all(ref["grad_image"][~ref["cmask"]] == 0)
        g32 = colour_grad_f32(I, T, A, ALPHA_MIN, 0.8, scale)
        assert np.abs(g32 - ref["grad_image"]).max() <= 2.0 ** -22 * 0.8 * scale
        assert np.array_equal(np.sign(g32), np.sign(ref["grad_image"]))
    # the reference differentiates its own loss (central difference in double, away from the kinks and the masks' edges)
    I, D, A, T, z = loss_inputs(7, 9, 3)
    args = (ALPHA_MIN, 0.8, 1.3, 0.0, 0.25)
    ref = track_loss_f64(I, D, A, T, z, *args)
    h = 1e-6
    for (y, x) in zip(*np.nonzero(ref["dmask"])):
        for name, arr in (("grad_depth", D), ("grad_alpha", A)):
            if abs(ref["r"][y, x]) < 1e-3 or abs(A[y, x] - 0.5) < 1e-3:
                continue
            p, m = arr.astype(np.float64), arr.astype(np.float64)
            p[y, x] += h
            m[y, x] -= h
            lp = track_loss_f64(I, p if arr is D else D, p if arr is A else A, T, z, *args)["loss"]
            lm = track_loss_f64(I, m if arr is D else D, m if arr is A else A, T, z, *args)["loss"]
            assert abs((lp - lm) / (2 * h) - ref[name][y, x]) <= 1e-6 * abs(ref[name][y, x]) + 1e-9, (name, y, x)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


# VGPRs / LDS bytes as the build reports them: the streaming kernel holds four pixels' twelve image
# and twelve target floats, D, A, z and the twenty gradients of one lane -- 53 with a range map, 39 without; the finalize
# kernel's last thread adds 16 x 3 doubles from LDS, unrolled -- 55.  All of them leave eight waves per SIMD.
TRACK_KERNELS = {"track_loss_kernelILb1EE": (53, 48), "track_loss_kernelILb0EE": (39, 48), "track_loss_finalize_kernel": (55, 384)}


@pytest.mark.parametrize("part", list(TRACK_KERNELS))
def test_track_loss_kernels_resources(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    vgprs, lds = TRACK_KERNELS[part]
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch
    assert k[".vgpr_count"] == vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".group_segment_fixed_size"] == lds, (k[".name"], k[".group_segment_fixed_size"])
    assert k[".vgpr_count"] <= 64  # eight waves per SIMD
