"""CPU tier of RGB-D training (include/gs_abi.h: gs_loss_depth, gs_frame_backward_adam_aux): the three symbols and their
ctypes bindings, the depth loss's workspace size query and argument checks, every refusal of the fused aux step on fake
pointers (each comes before anything is enqueued), gs_frame_backward_adam's unchanged refusal of aux frames, the z -> range
conversion, and the register / scratch budgets of the new kernels read from the built code objects.  No kernel is launched."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from gs_testutil import FAKE, fake_adam as _adam, fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2


_frame = functools.partial(fake_frame, aux=True)


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_loss_depth_workspace_bytes", "gs_loss_depth", "gs_frame_backward_adam_aux"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("gs_loss_depth_workspace_bytes(", "int gs_loss_depth(", "int gs_frame_backward_adam_aux("):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays


def test_depth_loss_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_loss_depth_workspace_bytes
    sizes = [(48, 64), (187, 250), (480, 640), (1080, 1920), (2160, 3840)]
    got = [q(h, w) for h, w in sizes]
    for b in got:
        assert b > 0 and b % 256 == 0
    assert got == sorted(got) and got[-1] > got[0]  # monotone in H * W
    assert q(1, 1) > 0
    for bad in ((0, 64), (48, 0), (-1, 64), (48, -7), (0, 0)):
        assert q(*bad) == 0


def test_depth_loss_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    H, W = 48, 64
    ws_bytes = _lib.gs_loss_depth_workspace_bytes(H, W)
    D, A, Z, GD, GA, WS = (FAKE + i * (1 << 24) for i in range(6))

    def call(depth=D, alpha=A, target=Z, h=H, w=W, mode=0, amin=0.5, scale=1.0, gd=GD, ga=GA, ws=WS, nbytes=ws_bytes):
        return _lib.gs_loss_depth(depth, alpha, target, h, w, mode, amin, scale, gd, ga, None, ws, nbytes, None)

    for mode in (-1, 2, 7):
        assert call(mode=mode) == GS_E_INVALID
        assert b"mode" in _lib.gs_last_error()
    for kw in ("depth", "alpha", "target", "gd", "ga"):
        assert call(**{kw: None}) == GS_E_INVALID
        assert b"null" in _lib.gs_last_error()
    assert call(ws=None) == GS_E_INVALID
    assert call(nbytes=ws_bytes - 1) == GS_E_INVALID
    assert call(nbytes=0) == GS_E_INVALID
    assert b"workspace" in _lib.gs_last_error()
    assert call(h=0) == GS_E_INVALID and call(w=-3) == GS_E_INVALID
    assert call(depth=D + 4) == GS_E_INVALID  # the maps are walked float4 by float4
    assert call(mode=1, amin=0.0) == GS_E_INVALID  # the expected depth divides by alpha
    assert call(scale=float("nan")) == GS_E_INVALID


def test_fused_aux_step_refusals_come_before_any_launch():
    from gaussian import _lib

    call = _lib.gs_frame_backward_adam_aux
    gimg = FAKE + (8 << 30)
    # a frame without the flag: gs_frame_backward_adam is its entry point
    assert call(C.byref(_frame(aux=False)), gimg, C.byref(_adam()), None) == GS_E_INVALID
    assert b"GS_FRAME_AUX" in _lib.gs_last_error()
    # not a training frame
    assert call(C.byref(_frame(training=0)), gimg, C.byref(_adam()), None) == GS_E_INVALID
    assert b"training" in _lib.gs_last_error()
    # no optimizer descriptor
    assert call(C.byref(_frame()), gimg, None, None) == GS_E_INVALID
    # a descriptor gs_validate_adam_fused rejects: all-zero (step 0), a bad beta, a missing moment, a misaligned moment
    assert call(C.byref(_frame()), gimg, C.byref(_adam(good=False)), None) == GS_E_INVALID
    a = _adam()
    a.beta2 = 1.0
    assert call(C.byref(_frame()), gimg, C.byref(a), None) == GS_E_INVALID
    a = _adam()
    a.exp_avg_sq[3] = None
    assert call(C.byref(_frame()), gimg, C.byref(a), None) == GS_E_INVALID
    a = _adam()
    a.exp_avg[0] += 4
    assert call(C.byref(_frame()), gimg, C.byref(a), None) == GS_E_INVALID
    a = _adam()
    a.stat_mode = 1  # a statistic without its array
    assert call(C.byref(_frame()), gimg, C.byref(a), None) == GS_E_INVALID
    # pose gradients are not part of the fused step (the refusal names the flag; SH colours alike)
    for cd in (3, 27):
        f = _frame(color_dim=cd)
        f.flags |= _lib.GS_FRAME_POSE_GRAD
        f.grad_rot, f.grad_tran = FAKE + (9 << 30), FAKE + (9 << 30) + 64
        f.pose_workspace = FAKE + (10 << 30)
        f.pose_workspace_bytes = _lib.gs_frame_pose_workspace_bytes(f.N)
        assert call(C.byref(f), gimg, C.byref(_adam()), None) == GS_E_UNSUPPORTED
        assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()
    # an invalid description is caught first
    f = _frame()
    f.aux_padded = None
    assert call(C.byref(f), gimg, C.byref(_adam()), None) == GS_E_INVALID


def test_plain_fused_step_still_refuses_aux_frames():
    from gaussian import _lib

    rc = _lib.gs_frame_backward_adam(C.byref(_frame(aux=True)), FAKE + (8 << 30), C.byref(_adam()), None)
    assert rc == GS_E_UNSUPPORTED
    assert b"GS_FRAME_AUX" in _lib.gs_last_error()


def test_train_options_and_depth_loss_class_exist():
    import gs_train

    o = gs_train.TrainOptions()
    assert (o.depth_weight, o.depth_mode, o.depth_alpha_min) == (0.0, "residual", 0.5)
    assert gs_train.DepthLoss.MODES == {"residual": 0, "expected": 1}
    with pytest.raises(RuntimeError):
        gs_train.DepthLoss(48, 64, "residual", 0.5, "cpu")  # a HIP kernel: no CPU fallback
    with pytest.raises(ValueError):
        gs_train.DepthLoss(48, 64, "huber", 0.5, "cpu")


def test_z_to_range_uses_the_renderers_pixel_centres():
    """range = z |ray| / ray_z per pixel of the CROPPED image: for an axis-aligned camera the ray of padded pixel (px, py) is
    ((px - padW / 2 + 0.5) / fx, (py - padH / 2 + 0.5) / fy, 1) (splatter.RayInfo), and a rotation of the camera changes nothing."""
    import torch
    from gs_scene import make_camera
    from gs_train import z_to_range

    for W, H in ((250, 187), (64, 48)):
        padW, padH = -(-W // 16) * 16, -(-H // 16) * 16
        top, left = (padH - H) // 2, (padW - W) // 2
        z = torch.from_numpy(np.random.default_rng(0).uniform(0.5, 9.0, (H, W)).astype(np.float32))
        z[3, 5], z[7, 1] = 0.0, float("inf")
        for yaw in (0.0, 25.0):
            cam = make_camera(W, H, yaw_deg=yaw)
            x = (np.arange(W) + left - padW / 2 + 0.5) / float(cam.focal_x)
            y = (np.arange(H) + top - padH / 2 + 0.5) / float(cam.focal_y)
            want = z.numpy().astype(np.float64) * np.sqrt(x[None, :] ** 2 + y[:, None] ** 2 + 1.0)
            got = z_to_range(z, cam).numpy().astype(np.float64)
            assert got[3, 5] == 0.0 and np.isinf(got[7, 1])
            ok = np.isfinite(want)
            assert np.abs(got[ok] - want[ok]).max() <= 4e-6 * want[ok].max(), (W, H, yaw)


# ---------------------------------------------------------------------------------------------------------------------
# Register / scratch budgets of the new kernels (the read-out of tests/test_kernel_resources.py).  The aux variants of the
# fused step carry the depth term's row walk next to their twin's live state: VGPR counts as the build reports them
#  -- rgb 77 (twin 75: six waves per SIMD, as the twin), degree 2 112 (twin 106: four waves, as the
# twin), degree 3 98 (twin 91: the register file would hold five waves of the twin and four of the variant, but 17 KiB of LDS
# per two-wave workgroup admit nine workgroups per CU, 4.5 waves per SIMD, either way) --, no scratch, the twin's LDS.
AUX_ADAM_VGPRS = {("3", "256"): 77, ("27", "128"): 112, ("48", "128"): 98}


@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def _pick(d, parts):
    hits = [k for k in d if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits)
    return d[hits[0]]


@pytest.mark.parametrize("cd,blk", list(AUX_ADAM_VGPRS), ids=[f"C{c}" for c, _ in AUX_ADAM_VGPRS])
@pytest.mark.parametrize("mode", ("1", "2"))
def test_aux_adam_variant_against_its_twin(kernels, cd, blk, mode):
    aux = _pick(kernels, (f"frame_project_backward_adam_aux_kernelILi{cd}ELi{blk}ELi{mode}EE",))
    twin = _pick(kernels, (f"frame_project_backward_kernelILi{cd}ELi0ELi{blk}ELi{mode}EE",))
    assert aux[".vgpr_count"] == AUX_ADAM_VGPRS[(cd, blk)], (aux[".name"], aux[".vgpr_count"])
    assert aux[".private_segment_fixed_size"] <= twin[".private_segment_fixed_size"]
    assert aux[".vgpr_spill_count"] <= twin[".vgpr_spill_count"]
    assert aux[".private_segment_fixed_size"] == 0 and aux[".vgpr_spill_count"] == 0
    assert aux[".group_segment_fixed_size"] == twin[".group_segment_fixed_size"]


@pytest.mark.parametrize("parts,vgprs", [(("depth_loss_kernelILi0E",), 32), (("depth_loss_kernelILi1E",), 32),
                                         (("depth_loss_finalize_kernel",), 32)])
def test_depth_loss_kernels_are_small(kernels, parts, vgprs):
    k = _pick(kernels, parts)
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
