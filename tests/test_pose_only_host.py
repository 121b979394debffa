"""CPU tier of the pose-only backward (gs_frame_backward_pose, include/gs_abi.h): the export and its binding, every refusal in
the order the header states -- on fake pointers, so nothing here can have been enqueued --, the unchanged refusals of
gs_frame_backward_part, the Tracker's option, and the resources of the two frame_pose_backward_kernel instantiations read from
the built code object against those of the fused step's pose kernel, whose work they do a strict subset of."""
import ctypes as C
import os
import re

import pytest

from gs_testutil import FAKE
from test_pose_host import GS_E_INVALID, GS_E_UNSUPPORTED, _frame, _grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    from gaussian import _lib

    return _lib.gs_last_error().decode()


def test_symbol_is_exported_bound_and_declared():
    from gaussian import _lib

    assert "gs_frame_backward_pose" in _lib.EXPORTS
    assert getattr(_lib.lib, "gs_frame_backward_pose") is not None
    assert _lib.gs_frame_backward_pose.restype is C.c_int and len(_lib.gs_frame_backward_pose.argtypes) == 4
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    assert re.search(r"^int gs_frame_backward_pose\(const gs_frame \*f, const float \*grad_image, int32_t part, "
                     r"gs_stream_t stream\);$", header, re.M)
    assert _lib.gs_abi_version() == 8  # additive


def test_refusals_come_in_the_stated_order():
    from gaussian import _lib

    call = _lib.gs_frame_backward_pose
    GEO = _lib.GS_BWD_GEOMETRY
    # 1. validate(f): the pose fields as everywhere -- ahead of everything else that is wrong with the call
    for field in ("pose_workspace", "grad_rot", "grad_tran"):
        f = _frame(training=0, color_dim=27)
        setattr(f, field, None)
        assert call(C.byref(f), None, 7, None) == GS_E_INVALID
        assert "training forward" not in _err() and "part must" not in _err()
    f = _frame()
    f.pose_workspace_bytes -= 256
    assert call(C.byref(f), FAKE, 0, None) == GS_E_INVALID and "pose workspace too small" in _err()
    # 2. not a training frame -- ahead of a bad part, a missing flag, SH colours and a NULL image
    for f in (_frame(training=0, color_dim=27), _frame(training=0, pose=False)):
        assert call(C.byref(f), None, 7, None) == GS_E_INVALID
        assert "training forward" in _err()
    f = _frame()
    f.image_padded = None
    assert call(C.byref(f), FAKE, 0, None) == GS_E_INVALID and "training forward" in _err()
    # 3. the part -- ahead of a missing flag, SH colours and a NULL image
    for part in (_lib.GS_BWD_RASTER, _lib.GS_BWD_COLOR, GEO | _lib.GS_BWD_COLOR, -1, 7):
        for f in (_frame(pose=False), _frame(color_dim=48), _frame()):
            assert call(C.byref(f), None, part, None) == GS_E_INVALID
            assert "part must be 0 or GS_BWD_GEOMETRY" in _err()
    # 4. a frame without the flag -- ahead of SH colours and a NULL image; the message names the flag
    for part in (0, GEO):
        for f in (_frame(pose=False), _frame(pose=False, aux=True), _frame(pose=False, color_dim=27)):
            assert call(C.byref(f), None, part, None) == GS_E_INVALID
            assert "not flagged GS_FRAME_POSE_GRAD" in _err()
    # 5. SH colours: the sentence every backward of such a frame answers with -- ahead of a NULL image
    for cd in (27, 48):
        for part in (0, GEO):
            assert call(C.byref(_frame(color_dim=cd)), None, part, None) == GS_E_UNSUPPORTED
            assert _err().startswith("gs_frame_backward_pose: GS_FRAME_POSE_GRAD needs rgb colours (color_dim 3)")
    # 6. a NULL image with part 0, plain and aux frames (GS_BWD_GEOMETRY does not read it: nothing left to refuse there,
    # and with fake pointers nothing more may be called)
    for f in (_frame(), _frame(aux=True)):
        assert call(C.byref(f), None, 0, None) == GS_E_INVALID
        assert _err() == "gs_frame_backward_pose: invalid argument: null pointer"


def test_backward_part_refuses_a_flagged_sh_frame_as_before():
    from gaussian import _lib

    for cd in (27, 48):
        f = _frame(color_dim=cd)
        for part in (_lib.GS_BWD_RASTER, _lib.GS_BWD_GEOMETRY, _lib.GS_BWD_COLOR):
            assert _lib.gs_frame_backward_part(C.byref(f), FAKE, *_grads(), part, None) == GS_E_UNSUPPORTED
            assert _err().startswith("gs_frame_backward: GS_FRAME_POSE_GRAD needs rgb colours")
    assert _lib.gs_frame_backward_part(C.byref(_frame()), FAKE, *_grads(), 0, None) == GS_E_INVALID
    assert "part must be GS_BWD_RASTER, GS_BWD_GEOMETRY or GS_BWD_COLOR" in _err()


def test_track_options_default_is_off():
    from gs_slam import SlamOptions
    from gs_track import TrackOptions

    assert TrackOptions().pose_only is False
    assert SlamOptions().track == TrackOptions()
    assert TrackOptions(pose_only=True) != TrackOptions()


# ------------------------------------------------------------------------------------------------------ kernel resources
@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def _only(kernels, *parts):
    hits = [k for k in kernels if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits)
    return kernels[hits[0]]


def test_exactly_two_instantiations(kernels):
    names = sorted(k for k in kernels if "frame_pose_backward_kernel" in k)
    assert len(names) == 2 and "frame_pose_backward_kernelILb0E" in names[0] and "frame_pose_backward_kernelILb1E" in names[1], names


@pytest.mark.parametrize("aux", [0, 1])
def test_pose_only_kernel_needs_no_more_than_the_fused_pose_step(kernels, aux):
    """No scratch, no spills, 256 threads; VGPRs and LDS at most those of frame_project_backward_adam_pose_kernel<AUX, 1> from the
    same code object (row sums + pose terms + the optimizer step: a superset of this kernel's work)."""
    k = _only(kernels, f"frame_pose_backward_kernelILb{aux}E")
    fused = _only(kernels, f"frame_project_backward_adam_pose_kernelILb{aux}ELi1E")
    print(f"frame_pose_backward_kernel<{aux}>: {k['.vgpr_count']} VGPRs, {k['.sgpr_count']} SGPRs, "
          f"{k['.group_segment_fixed_size']} bytes of LDS (fused pose step: {fused['.vgpr_count']} VGPRs, "
          f"{fused['.group_segment_fixed_size']} bytes)")
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_count"] <= fused[".vgpr_count"]
    assert k[".group_segment_fixed_size"] <= fused[".group_segment_fixed_size"]
