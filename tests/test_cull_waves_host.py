"""Host tier (no GPU): the budgets of the two project kernels of an occlusion-culled frame (cull_project.hip:
frame_project_cull_count_kernel, frame_packed_project_cull_count_kernel), read from a code object compiled here with the
project's own flags.  The kernels run one workgroup of 1,024 threads = 16 waves per CU: four waves per SIMD need <= 128 VGPRs;
every wave keeps three rounds of phase A and one drain's survivors in registers, so a spill would sit in the stream; and the
static LDS (the tile-order workgroup's bins) plus the dynamic room the launch may ask for must fit the CU's 160 KiB."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "3d-gaussian-splatting_amd")
sys.path[:0] = [p for p in (PKG, os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]

GS_BIN_LDS_BYTES = 160000           # gs_frame_layout.h
ROOM = GS_BIN_LDS_BYTES - 8 * 4096  # the dynamic LDS gs_stage_project may ask for (hipFuncAttributeMaxDynamicSharedMemorySize)
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import gs_build
    from test_kernel_resources import code_objects, kernel_metadata

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    obj = str(tmp_path_factory.mktemp("cull_waves") / "cull_project.o")
    subprocess.check_call([hipcc, *gs_build.COMMON, *gs_build.SOURCES["cull_project.hip"], "-c",
                           os.path.join(gs_build.CSRC, "cull_project.hip"), "-o", obj])
    out = {}
    for elf in code_objects(open(obj, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


@pytest.mark.parametrize("name", ["frame_project_cull_count_kernel", "frame_packed_project_cull_count_kernel"])
def test_cull_kernel_budgets(kernels, name):
    hits = [v for k, v in kernels.items() if name in k]
    assert len(hits) == 1, (name, [h[".name"] for h in hits])
    k = hits[0]
    print(name, "VGPRs", k[".vgpr_count"], "scratch", k[".private_segment_fixed_size"], "static LDS", k[".group_segment_fixed_size"])
    assert k[".vgpr_count"] <= 128, k[".vgpr_count"]  # four waves per SIMD: the 1,024-thread workgroup launches
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".max_flat_workgroup_size"] == 1024
    assert k[".group_segment_fixed_size"] + ROOM <= CU_LDS, k[".group_segment_fixed_size"]


def test_ring_and_tail_fit_the_room_the_cull_rule_reserves():
    """gs_frame_occlusion_cull admits a frame when histogram + pyramid + 2 x 16,384 + 16 bytes fit the room: the rings of the 16
    waves (128 slots each) and the pooled tail (16 x 63 entries) must not take more than that reserve."""
    assert 4 * (16 * 128 + 16 * 63) <= 2 * 16384 + 16
