"""CPU tier of the depth / alpha maps (GS_FRAME_AUX, include/gs_abi.h): the aux workspace size query, the validation of a
flagged frame, the refusal of the fused-Adam backward, and the register / scratch budgets of the aux kernels read from the
built code objects.  No kernel is launched here."""
import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2


def _frame(aux=False, training=1, W=128, H=96):
    """A well-formed frame descriptor with fake (never dereferenced) device addresses: only host-side entry points that
    validate and return before any launch may be called with it."""
    from gaussian import _lib

    f = _lib.GsFrame()
    f.N, f.color_dim, f.scale_activation = 1000, 3, 0
    fake = 1 << 40
    f.pos, f.quat, f.scale, f.opa, f.rgb = fake, fake + 4096, fake + 8192, fake + 12288, fake + 16384
    f.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    f.near_plane, f.half_width, f.half_height = 0.01, 1.0, 1.0
    f.width, f.height, f.focal_x, f.focal_y = W, H, 0.75 * W, 0.75 * W
    f.thresh, f.max_pairs, f.sort_mode, f.tile_culling_method = 0.05, 50_000, 2, 2
    f.workspace = fake + (1 << 30)
    f.workspace_bytes = _lib.gs_frame_workspace_bytes(f.N, f.max_pairs, W, H, 3, training)
    f.training = training
    f.image, f.image_padded = fake + (2 << 30), fake + (3 << 30)
    if aux:
        f.flags = _lib.GS_FRAME_AUX
        f.aux_workspace = fake + (4 << 30)
        f.aux_workspace_bytes = _lib.gs_frame_aux_workspace_bytes(f.max_pairs, W, H, training)
        f.aux_padded = fake + (5 << 30)
    return f


def test_aux_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_frame_aux_workspace_bytes
    assert _lib.GS_FRAME_AUX == 2048
    for tr in (0, 1):
        assert q(1000, 64, 48, tr) > 0
        assert q(1000, 64, 48, tr) % 256 == 0
        assert q(2_000_000, 64, 48, tr) >= q(1000, 64, 48, tr)       # monotone in the pair capacity
        assert q(1000, 1920, 1080, tr) >= q(1000, 64, 48, tr)        # ... and in the image size
    assert q(2_000_000, 64, 48, 1) > q(1000, 64, 48, 1)
    assert q(1000, 1920, 1080, 1) > q(1000, 64, 48, 1)
    assert q(100_000, 640, 480, 1) > q(100_000, 640, 480, 0)         # the checkpoints are kept by training frames only
    # the (D, A) checkpoints: 8 bytes x 256 pixels per bucket of the capacity
    T = (640 // 16) * (480 // 16)
    assert q(100_000, 640, 480, 1) >= 8 * 256 * (100_000 // 64 + T + 1)
    for bad in ((-1, 64, 48, 1), (1000, 0, 48, 1), (1000, 64, 0, 0), (1000, -5, 48, 0)):
        assert q(*bad) == 0
    # the main workspace does not depend on the flag (its size query has no aux argument at all)
    assert _lib.gs_frame_workspace_bytes(1000, 50_000, 128, 96, 3, 1) > 0


def test_flagged_frame_validation_is_host_only():
    from gaussian import _lib

    # gs_frame_binning_variant validates the description and answers on the host (negative: does not validate)
    assert _lib.gs_frame_binning_variant(C.byref(_frame())) >= 0
    assert _lib.gs_frame_binning_variant(C.byref(_frame(aux=True))) >= 0
    assert _lib.gs_frame_binning_variant(C.byref(_frame(aux=True, training=0))) >= 0
    f = _frame(aux=True)
    f.aux_workspace = None
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    assert b"aux" in _lib.gs_last_error()
    f = _frame(aux=True)
    f.aux_workspace_bytes -= 256
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    assert b"aux workspace too small" in _lib.gs_last_error()
    f = _frame(aux=True)
    f.aux_workspace += 16  # not 256-byte aligned
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    f = _frame(aux=True)
    f.aux_padded = None  # a training frame's backward reads the raw sums
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    f = _frame(aux=True, training=0)
    f.aux_padded = None  # ... an inference frame needs none
    assert _lib.gs_frame_binning_variant(C.byref(f)) >= 0
    # an all-zero descriptor with the flag: rejected, nothing launched
    z = _lib.GsFrame()
    z.flags = _lib.GS_FRAME_AUX
    assert _lib.gs_frame_forward(C.byref(z), None) == GS_E_INVALID
    assert _lib.gs_frame_backward(C.byref(z), None, None, None, None, None, None, None) == GS_E_INVALID


def test_fused_adam_backward_refuses_aux_frames():
    from gaussian import _lib

    adam = _lib.GsAdamFused()
    rc = _lib.gs_frame_backward_adam(C.byref(_frame(aux=True)), 1 << 41, C.byref(adam), None)
    assert rc == GS_E_UNSUPPORTED
    assert b"GS_FRAME_AUX" in _lib.gs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Register / scratch budgets of the aux kernels (the read-out of tests/test_kernel_resources.py).  Limits proposed from the
# built code objects: rgb forward 140 / 142 VGPRs (three waves per SIMD: the four accumulators and the staged depth do not
# fit the plain kernel's 128), degree 2 at its plain kernel's 168 with a few spills outside the loop, degree 3 at 256
# without scratch; backward rgb 116 (four waves), degree 2 168 (three waves, a few spills outside the per-Gaussian loop) and
# degree 3 255 (two waves: one step below the plain kernels, whose budgets spilled inside the loop here);
# the per-Gaussian depth sums 26 VGPRs.
AUX_BUDGETS = [
    (("raster_aux_forward_kernelILi3ELb0E",), 168, False),
    (("raster_aux_forward_kernelILi3ELb1E",), 168, False),
    (("raster_aux_forward_kernelILi27ELb0E",), 168, True),
    (("raster_aux_forward_kernelILi27ELb1E",), 168, True),
    (("raster_aux_forward_kernelILi48ELb0E",), 256, True),
    (("raster_aux_forward_kernelILi48ELb1E",), 256, True),
    (("raster_aux_backward_kernelILi3E",), 128, False),
    (("raster_aux_backward_kernelILi27E",), 168, True),
    (("raster_aux_backward_kernelILi48E",), 256, True),
    (("frame_aux_depth_backward_kernelILi3E",), 64, False),
    (("frame_aux_depth_backward_kernelILi27E",), 64, False),
    (("frame_aux_depth_backward_kernelILi48E",), 64, False),
]
AUX_HOT_LOOPS = [
    (("raster_aux_forward_kernelILi3ELb0E",), "v_exp_f32", 8),
    (("raster_aux_forward_kernelILi3ELb1E",), "v_exp_f32", 8),
    (("raster_aux_forward_kernelILi27ELb0E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi27ELb1E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi48ELb0E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi48ELb1E",), "v_exp_f32", 32),
    (("raster_aux_backward_kernelILi3E",), "v_exp_f32", 4),
    (("raster_aux_backward_kernelILi27E",), "v_exp_f32", 4),
    (("raster_aux_backward_kernelILi48E",), "v_exp_f32", 4),
]


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
    return hits[0]


@pytest.mark.parametrize("parts,vgprs,scratch_ok", AUX_BUDGETS, ids=[b[0][0] for b in AUX_BUDGETS])
def test_aux_kernel_fits_its_register_budget(kernels, parts, vgprs, scratch_ok):
    k = kernels[_pick(kernels, parts)]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    if not scratch_ok:
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k[".name"]


def test_aux_kernels_keep_their_lds_budgets(kernels):
    # rgb forward: 16 one-wave workgroups per CU fit the LDS; rgb backward: four waves per SIMD
    assert kernels[_pick(kernels, ("raster_aux_forward_kernelILi3ELb0E",))][".group_segment_fixed_size"] * 16 <= 160 * 1024
    assert kernels[_pick(kernels, ("raster_aux_backward_kernelILi3E",))][".group_segment_fixed_size"] * 16 <= 160 * 1024


@pytest.fixture(scope="module")
def disassembly():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loops
    from test_kernel_resources import LIB

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    if not (os.path.exists(isa_loops.OBJDUMP) or shutil.which(isa_loops.OBJDUMP)):
        pytest.skip("llvm-objdump not found")
    return isa_loops, isa_loops.disassemble_library()


@pytest.mark.parametrize("parts,marker,at_least", AUX_HOT_LOOPS, ids=[h[0][0] for h in AUX_HOT_LOOPS])
def test_aux_hot_loop_is_free_of_scratch_instructions(disassembly, parts, marker, at_least):
    isa, dis = disassembly
    insns = dis[_pick(dis, parts)]
    cands = [(lo, hi) for lo, hi in isa.loops(insns) if isa.count(insns, lo, hi, marker) >= at_least]
    assert cands, (parts, "no loop with", at_least, marker)
    inner = [(lo, hi) for lo, hi in cands if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in cands)]
    for lo, hi in inner:
        assert isa.count(insns, lo, hi, "scratch_") == 0, (parts, lo, hi)
