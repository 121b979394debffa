"""CPU tier of the camera pose gradients (GS_FRAME_POSE_GRAD, include/gs_abi.h): the pose workspace size query, the validation
of a flagged frame, the refusals (SH colours, the slice and fused-Adam backwards), the ctypes mirror of the descriptor's new
trailing fields, and the register / scratch budgets of the new kernels read from the built code objects.  No kernel is
launched here: every call below is refused or answered on the host before anything is enqueued."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import pytest

from gs_testutil import FAKE, fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2


_frame = functools.partial(fake_frame, pose=True)


def _grads():
    return [FAKE + (8 << 30) + k * (1 << 24) for k in range(5)]


def test_pose_flag_value():
    from gaussian import _lib

    assert _lib.GS_FRAME_POSE_GRAD == 4096
    assert _lib.GS_FRAME_POSE_GRAD & (_lib.GS_FRAME_AUX | _lib.GS_FRAME_CULL_DILATE_NEAR) == 0


def test_pose_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_frame_pose_workspace_bytes
    sizes = [q(n) for n in (0, 1, 255, 256, 257, 5000, 376_467, 2_400_000, 1 << 30)]
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes)  # monotone in N
    # one 12-float row per 256 Gaussians for the projection backward and one for the aux depth kernel
    assert q(2_400_000) >= 2 * 48 * (2_400_000 // 256)
    assert q(-1) == 0 and q(-(1 << 40)) == 0


def test_flagged_frame_validation_is_host_only():
    from gaussian import _lib

    v = _lib.gs_frame_binning_variant
    assert v(C.byref(_frame())) >= 0
    assert v(C.byref(_frame(aux=True))) >= 0
    assert v(C.byref(_frame(training=0))) >= 0
    f = _frame()
    f.pose_workspace = None
    assert v(C.byref(f)) == GS_E_INVALID
    assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()
    f = _frame()
    f.pose_workspace_bytes -= 256
    assert v(C.byref(f)) == GS_E_INVALID
    assert b"pose workspace too small" in _lib.gs_last_error()
    f = _frame()
    f.pose_workspace += 16  # not 256-byte aligned
    assert v(C.byref(f)) == GS_E_INVALID
    f = _frame()
    f.grad_rot = None
    assert v(C.byref(f)) == GS_E_INVALID
    f = _frame()
    f.grad_tran = None
    assert v(C.byref(f)) == GS_E_INVALID
    # without the flag the trailing fields are not read at all
    f = _frame(pose=False)
    f.grad_rot = f.grad_tran = f.pose_workspace = None
    assert v(C.byref(f)) >= 0
    # the backward entry points validate the same way before anything else
    f = _frame()
    f.pose_workspace = None
    assert _lib.gs_frame_backward(C.byref(f), FAKE, *_grads(), None) == GS_E_INVALID
    assert _lib.gs_frame_backward_part(C.byref(f), None, *_grads(), _lib.GS_BWD_GEOMETRY, None) == GS_E_INVALID


def test_sh_frames_are_refused():
    from gaussian import _lib

    for cd in (27, 48):
        f = _frame(color_dim=cd)
        assert _lib.gs_frame_binning_variant(C.byref(f)) >= 0  # a valid description (forwards ignore the flag) ...
        assert _lib.gs_frame_backward(C.byref(f), FAKE, *_grads(), None) == GS_E_UNSUPPORTED  # ... no backward
        assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()
        for part in (_lib.GS_BWD_RASTER, _lib.GS_BWD_GEOMETRY, _lib.GS_BWD_COLOR):
            assert _lib.gs_frame_backward_part(C.byref(f), FAKE, *_grads(), part, None) == GS_E_UNSUPPORTED
    f = _frame(color_dim=27)
    ms = (C.c_float * 3)()
    assert _lib.gs_frame_backward_profile(C.byref(f), FAKE, *_grads(), ms, None) == GS_E_UNSUPPORTED


def test_slice_backward_is_refused():
    from gaussian import _lib

    f = _frame()
    for part in (_lib.GS_BWD_GEOMETRY, _lib.GS_BWD_COLOR, _lib.GS_BWD_GEOMETRY | _lib.GS_BWD_COLOR):
        rc = _lib.gs_frame_backward_slice(C.byref(f), *_grads(), part, 0, 256, None)
        assert rc == GS_E_UNSUPPORTED
        assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()


def test_fused_adam_backward_is_refused():
    from gaussian import _lib

    adam = _lib.GsAdamFused()
    assert _lib.gs_frame_backward_adam(C.byref(_frame()), FAKE, C.byref(adam), None) == GS_E_UNSUPPORTED
    assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gs_abi.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gs_frame), offsetof(gs_frame, depth),
           offsetof(gs_frame, alpha), offsetof(gs_frame, aux_padded), offsetof(gs_frame, aux_workspace),
           offsetof(gs_frame, aux_workspace_bytes), offsetof(gs_frame, grad_depth), offsetof(gs_frame, grad_alpha),
           offsetof(gs_frame, grad_rot), offsetof(gs_frame, grad_tran), offsetof(gs_frame, pose_workspace),
           offsetof(gs_frame, pose_workspace_bytes));
    return 0;
}
"""


def test_ctypes_descriptor_matches_the_header(tmp_path):
    from gaussian import _lib

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on PATH")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(_LAYOUT_C)
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = _lib.GsFrame
    want = [C.sizeof(G)] + [getattr(G, n).offset for n in ("depth", "alpha", "aux_padded", "aux_workspace",
                                                            "aux_workspace_bytes", "grad_depth", "grad_alpha", "grad_rot",
                                                            "grad_tran", "pose_workspace", "pose_workspace_bytes")]
    assert got == want
    assert [n for n, _ in G._fields_][-4:] == ["grad_rot", "grad_tran", "pose_workspace", "pose_workspace_bytes"]


# ---------------------------------------------------------------------------------------------------------------------
# Register / scratch budgets of the new kernels (the read-out of tests/test_kernel_resources.py).  Limits proposed from the
# first build: the pose variant of the rgb projection backward 76 VGPRs (PART 0) / 70 (PART 1) against the plain kernel's 67
# -- at most 80 keeps the plain kernel's six waves per SIMD --, the aux depth pose variant 30, the finalize kernel 106 (one
# workgroup of 1,024 threads: 128 is the hard limit).  No scratch anywhere.
POSE_BUDGETS = [
    (("frame_project_backward_pose_kernelILi0E",), 80),
    (("frame_project_backward_pose_kernelILi1E",), 80),
    (("frame_aux_depth_pose_backward_kernel",), 40),
    (("pose_grad_finalize_kernel",), 128),
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


@pytest.mark.parametrize("parts,vgprs", POSE_BUDGETS, ids=[b[0][0] for b in POSE_BUDGETS])
def test_pose_kernel_fits_its_register_budget(kernels, parts, vgprs):
    k = kernels[_pick(kernels, parts)]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k[".name"]


def test_pose_kernels_keep_the_lds_budget(kernels):
    # the pose sum adds 192 bytes to the plain kernel's LDS: still six workgroups of 256 per CU
    plain = kernels[_pick(kernels, ("frame_project_backward_kernelILi3ELi0ELi256ELi0E",))][".group_segment_fixed_size"]
    pose = kernels[_pick(kernels, ("frame_project_backward_pose_kernelILi0E",))][".group_segment_fixed_size"]
    assert pose <= plain + 256 and pose * 6 <= 160 * 1024


def test_plain_kernel_names_are_picked_once(kernels):
    # the substrings the existing budgets pick by still match exactly one kernel each
    for parts in (("frame_project_backward_kernelILi3ELi0ELi256ELi0E",), ("frame_project_backward_kernelILi3ELi0ELi256ELi1E",),
                  ("frame_aux_depth_backward_kernelILi3E",)):
        _pick(kernels, parts)
