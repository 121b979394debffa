"""Build recipe for libgs_amd.so (hipcc, gfx950 only, in-tree).

``python gs_build.py`` or ``build()``: every ``csrc/*.hip`` is compiled to an object with
``hipcc --offload-arch=gfx950 -O3`` and linked into ``csrc/libgs_amd.so``.  Files whose results
feed the integer side of the pipeline (depth bits, tile rectangles: cull_project.hip, binning.hip) are
compiled with ``-ffp-contract=off`` so they match the oracle bit for bit; the other files that carry the
flag say why beside their entry in ``SOURCES``.
No torch / pybind dependency: the library is a plain C ABI (include/gs_abi.h).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libgs_amd.so")

SOURCES = {
    # no SLP packing: the packer turns the 3x3 products into v_pk_mul/v_pk_add + ~140 v_mov shuffles per Gaussian;
    # a packed op has no rate advantage on gfx950, so that is pure issue time (and 66 instead of 45 VGPRs)
    "cull_project.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # uncontracted because the backward is pinned bit for bit by the golden tests, the fused step rounds like adam.hip,
    # and the AUX position term is fl(gp) + gpa in that order (project_backward / pose_terms contract by pragma);
    # no SLP packing, as above
    "project_bwd.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "binning.hip": ["-ffp-contract=off"],
    "radix_sort.hip": [],
    "tile_sort.hip": [],
    "tile_bin.hip": [],
    "strip_bin.hip": [],
    # no SLP packing: v_pk_*_f32 has no rate advantage on gfx950 and costs extra v_mov shuffles
    "raster_fwd.hip": ["-fno-slp-vectorize"],
    "raster_fwd_ref.hip": ["-fno-slp-vectorize"],  # the same kernel (raster_fwd_body.h), built the same way
    "raster_fwd_segment.hip": ["-fno-slp-vectorize"],  # its steps restated for the segments of a long list, as above
    "raster_bwd.hip": ["-fno-slp-vectorize"],
    "raster_bwd_systolic.hip": ["-fno-slp-vectorize"],
    "raster_bwd_pixel.hip": ["-fno-slp-vectorize"],
    "raster_bwd_mfma.hip": ["-fno-slp-vectorize"],
    "raster_bwd_rows.hip": ["-fno-slp-vectorize"],
    "gs_frame.hip": [],
    "adam.hip": ["-ffp-contract=off"],  # same roundings as torch's unfused elementwise kernels
    "loss.hip": ["-fno-slp-vectorize"],  # as above: the packer costs ~50 v_mov per row step of the fused kernel
    "densify.hip": ["-ffp-contract=off"],
    "seed.hip": ["-ffp-contract=off"],  # z A < (1 - front_rel) D as written: a float32 restatement decides identically
    # r = D - A z, r = D / A - z and the gate as written: one rounding per operation, and gs_loss_track's depth term is
    # gs_loss_depth mode 1 bit for bit
    "map_loss.hip": ["-ffp-contract=off"],
    # the per-pixel terms of map_loss.hip (map_terms.h) with the same roundings: where a term counts, gs_loss_track_gated's
    # gradients are gs_loss_track's bit for bit, and the thresholds are fl(k m) as written
    "track_gate.hip": ["-ffp-contract=off"],
    # the seen / not seen test as written: a float32 restatement decides identically; no SLP packing, as above
    "overlap.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # overlap.hip's decisions (overlap_point.h) under overlap.hip's flags: the same bits, counted per point
    "redundancy.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # the keep test (opa > t and ||act(scale)|| < s) as written: densify.hip's delete rule, decided identically
    "map_edit.hip": ["-ffp-contract=off"],
    # the row step of raster_bwd_rows.hip's kernel, built like it (no SLP packing, as above)
    "contrib.hip": ["-fno-slp-vectorize"],
    # the box sum, s / n and the edge test hi <= fl(fl(1 + edge_rel) lo) as written, one rounding per operation: the float32
    # restatement (tests/pyramid_ref.py) gives the level targets bit for bit
    "pyramid.hip": ["-ffp-contract=off"],
    # the vertices, the normals and the keep / drop tests of icp_point.h as written, one rounding per operation: the float32
    # restatement (tests/icp_ref.py) gives the maps bit for bit and the counts exactly; no SLP packing, as above
    "icp.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # Adam on the pose's six tangent numbers in double, every product rounded before it is added: the Python restatement
    # (tests/pose_step_ref.py) follows it operation by operation
    "pose_step.hip": ["-ffp-contract=off"],
    # I' = fl(fl(gain I) + bias) and g = fl(gain g') as written, the Adam step in double with every product rounded before
    # it is added: the restatement (tests/exposure_ref.py) gives the maps bit for bit and follows the step operation by
    # operation
    "exposure.hip": ["-ffp-contract=off"],
}
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall",
          "-Wno-unused-function", "-munsafe-fp-atomics",
          *os.environ.get("GS_EXTRA_HIPCC_FLAGS", "").split()]  # experiments only (-D switches)
HEADERS = ["gs_common.h", "gs_frame_layout.h", "project_common.h", "raster_common.h", "raster_bwd_common.h", "strip_common.h", "tile_bin_common.h",
           "raster_fwd_common.h", "raster_fwd_body.h",
           "frame_project_backward_body.inc", "aux_depth_backward_body.inc", "aux_depth_term.inc", "overlap_point.h",
           "seed_apply_body.inc", "overlap_count_body.inc", "map_terms.h", "icp_point.h", "loss_fused_body.inc",
           os.path.join("..", "..", "include", "gs_abi.h")]


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, outdir: str = None, defines=()) -> str:
    """Default: csrc/libgs_amd.so.  ``outdir`` + ``defines`` (-D switches) build an experiment VARIANT of the library
    somewhere else (tools/ab_variants.py; load it with GS_AMD_LIB=<path>): never the product build."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    objs, jobs = [], []
    odir = outdir or CSRC
    os.makedirs(odir, exist_ok=True)
    lib = os.path.join(odir, "libgs_amd.so")
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(odir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc, *COMMON, *extra, *defines, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(lib, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
