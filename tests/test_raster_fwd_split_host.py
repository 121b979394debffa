"""CPU tier of the forward compositing files (csrc/raster_fwd_common.h, raster_fwd_body.h, raster_fwd.hip, raster_fwd_ref.hip,
raster_fwd_segment.hip): the three sources are built with the same flags, an edit to either header makes the objects stale,
and the built library holds exactly the 65 forward kernels the three translation units instantiate between them -- the frame
path's 12 + 6, the reference API's 32 and the 15 of the segmented compositing -- with the frame kernels inside the register
budgets of tests/test_kernel_resources.py.  No kernel is launched."""
import os

import pytest

from test_kernel_resources import BUDGETS, LIB, code_objects, kernel_metadata, pick

FWD_SOURCES = ("raster_fwd.hip", "raster_fwd_ref.hip", "raster_fwd_segment.hip")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(LIB), "libgs_amd.so is not built"
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        md = kernel_metadata(elf)
        assert not set(md) & set(out), sorted(set(md) & set(out))  # no kernel is built in two translation units
        out.update(md)
    return out


def test_the_three_sources_are_built_alike_and_the_headers_are_dependencies():
    import gs_build

    flags = [gs_build.SOURCES[s] for s in FWD_SOURCES]
    assert flags[0] == flags[1] == flags[2] and "-fno-slp-vectorize" in flags[0]
    assert "raster_fwd_common.h" in gs_build.HEADERS and "raster_fwd_body.h" in gs_build.HEADERS
    for name in FWD_SOURCES + ("raster_fwd_common.h", "raster_fwd_body.h"):
        assert os.path.exists(os.path.join(gs_build.CSRC, name)), name


def count(kernels, part):
    return sum(part in k for k in kernels)


def test_the_library_holds_exactly_the_65_forward_kernels(kernels):
    assert count(kernels, "raster_forward_kernel") == 44
    assert count(kernels, "raster_aux_forward_kernel") == 6
    assert count(kernels, "raster_segment_kernel") == 12
    assert count(kernels, "seg_combine_kernel") == 2
    assert count(kernels, "seg_scan_kernel") == 1
    # <CDIM, FRAME, ...>: the frame path's 12 (rgb, degree 2, degree 3) and the reference API's 32 (rgb, degree 2)
    for cdim, n_frame, n_ref in ((3, 4, 16), (27, 4, 16), (48, 4, 0)):
        assert count(kernels, f"raster_forward_kernelILi{cdim}ELb1E") == n_frame
        assert count(kernels, f"raster_forward_kernelILi{cdim}ELb0E") == n_ref


FWD_BUDGETS = [b for b in BUDGETS if "raster_forward_kernel" in b[0][0]]  # 128 / 128 / 168 / 256 VGPRs


@pytest.mark.parametrize("parts,vgprs,scratch_ok", FWD_BUDGETS, ids=[b[0][0] for b in FWD_BUDGETS])
def test_the_frame_kernels_keep_their_register_budgets(kernels, parts, vgprs, scratch_ok):
    k = pick(kernels, *parts)
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    if not scratch_ok:
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k[".name"]
