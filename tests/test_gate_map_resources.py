"""CPU tier: the register / scratch budget of the weighted image-loss kernel and of the gate-mask kernels, read from the
gfx950 code objects inside the built libgs_amd.so as tests/test_kernel_resources.py reads them (no GPU, no recompilation)."""
import os

import pytest

from test_kernel_resources import LIB, code_objects, kernel_metadata


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def _one(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    return kernels[hits[0]]


def test_weighted_loss_kernel_fits_the_fused_kernels_budget(kernels):
    """loss_fused_kernel's own budget in test_kernel_resources.py: one workgroup of 512 per CU, two waves per SIMD -- at most
    256 VGPRs, no spills, no scratch.  The LDS is the unweighted kernel's: the weights are read from memory, not staged."""
    k, plain = _one(kernels, "loss_weighted_kernel"), _one(kernels, "loss_fused_kernel")
    print(f"loss_weighted_kernel: {k['.vgpr_count']} VGPRs (loss_fused_kernel {plain['.vgpr_count']}), "
          f"{k['.group_segment_fixed_size']} B LDS, {k['.sgpr_count']} SGPRs")
    assert k[".vgpr_count"] <= 256, k[".vgpr_count"]
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".group_segment_fixed_size"] == plain[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == 512
    assert "loss_fused_kernel" not in k[".name"]  # test_kernel_resources.py picks THE kernel of that name


@pytest.mark.parametrize("part", ["gate_mask_kernelILb1EE", "gate_mask_kernelILb0EE", "gate_mask_finalize_kernel",
                                  "l1_weighted_kernel"])
def test_gate_mask_kernels_have_no_scratch(kernels, part):
    k = _one(kernels, part)
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch
    assert k[".vgpr_count"] <= 128  # at least four waves per SIMD
    assert "track_gate_" not in k[".name"]  # test_track_gate_host.py counts the kernels of that prefix
