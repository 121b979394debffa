"""CPU tier of the covisibility count and the mapping loop's host logic (include/gs_abi.h: gs_view_overlap,
gs_view_overlap_workspace_bytes, gs_view_overlap_check_view; csrc/overlap_point.h; gs_slam.select_keyframes / is_keyframe):
the symbols and bindings, the workspace size query, every refusal on fake pointers (each comes before anything is enqueued),
the two restatements of tests/overlap_ref.py against each other and against closed forms on the cases the GPU tier uses, the
per-point header compiled for the host against the float32 restatement, the keyframe rules on hand-made counts, and the
resources of the two kernels read from the built code object.  No kernel is launched."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import overlap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splatting_amd", "csrc")
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 96, 128


def _opts(**kw):
    from gaussian import _lib

    o = _lib.GsOverlapOpts(2, 0.3, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _cam(**kw):
    from gaussian import _lib

    c = _lib.GsSeedCamera()
    c.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    c.focal_x = c.focal_y = 0.75 * W
    c.width, c.height = W, H
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_view_overlap_workspace_bytes", "gs_view_overlap_check_view", "gs_view_overlap"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_view_overlap_workspace_bytes(", "int gs_view_overlap(", "int gs_view_overlap_check_view(",
                 "} gs_overlap_opts;", "#define GS_OVERLAP_MAX_VIEWS 256", "cannot be validated here without a read"):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    assert C.sizeof(_lib.GsSeedCamera) == 64 and C.sizeof(_lib.GsOverlapOpts) == 12  # one line per view
    assert _lib.GS_OVERLAP_MAX_VIEWS == 256
    point = open(os.path.join(CSRC, "overlap_point.h")).read()
    assert "static_assert(sizeof(gs_seed_camera) == 64" in point and "__host__ __device__" in point
    import gs_build

    assert "overlap_point.h" in gs_build.HEADERS and "-ffp-contract=off" in gs_build.SOURCES["overlap.hip"]


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_view_overlap_workspace_bytes
    sizes = [(1, 1), (37, 53), (120, 160), (480, 640), (1080, 1920), (2160, 3840)]
    for n_views in (1, 3, 65, 256):
        got = [q(h, w, 1, n_views) for h, w in sizes]
        for b in got:
            assert b > 0 and b % 256 == 0
        assert got == sorted(got) and got[-1] > got[0]  # monotone in the image
    for h, w in sizes:
        by_views = [q(h, w, 1, n) for n in (1, 2, 64, 65, 255, 256)]
        assert by_views == sorted(by_views)  # ... in the views
        by_stride = [q(h, w, s, 256) for s in (1, 2, 3, 8)]
        assert by_stride == sorted(by_stride, reverse=True)  # ... and falling with the stride: fewer lattice pixels
    # a row of n_views + 2 uint32 per workgroup, at most 2,048 workgroups
    assert q(1080, 1920, 1, 256) <= 2048 * 258 * 4 + 256
    assert q(37, 53, 1, 65) == (8 * 67 * 4 + 255) // 256 * 256  # 1,961 lattice pixels: eight workgroups
    for bad in ((-1, 64, 1, 4), (48, 0, 1, 4), (48, 64, 0, 4), (48, 64, 1, 0), (48, 64, 1, 257)):
        assert q(*bad) == 0


def test_overlap_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    n_views = 5
    ws_bytes = _lib.gs_view_overlap_workspace_bytes(H, W, 2, n_views)
    Z, V, CNT, WS = (FAKE + i * (1 << 24) for i in range(4))

    def call(rng=Z, cam="default", views=V, n=n_views, opts="default", cnt=CNT, ws=WS, nbytes=ws_bytes):
        o = _opts() if opts == "default" else opts
        c = _cam() if cam == "default" else cam
        return _lib.gs_view_overlap(rng, C.byref(c) if c is not None else None, views, n,
                                    C.byref(o) if o is not None else None, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_view_overlap" in msg or b"overlap_check" in msg, msg
        assert word in msg, (kw, msg)

    for kw in ("rng", "cam", "views", "opts", "cnt"):
        refused(b"null", **{kw: None})
    for hw in (dict(width=0), dict(height=-3), dict(width=1 << 16, height=1 << 16)):
        refused(b"size", cam=_cam(**hw))
    for f in (0.0, -2.0, float("nan"), float("inf")):
        refused(b"focal", cam=_cam(focal_x=f))
        refused(b"focal", cam=_cam(focal_y=f))
    for s in (0, -1, -64):
        refused(b"stride", opts=_opts(stride=s))
    for v in (0.0, -0.3, float("nan"), float("inf")):
        refused(b"near", opts=_opts(near=v))
    for b in (-1, -100):
        refused(b"border", opts=_opts(border=b))
    for n in (0, -1, 257, 1 << 20):
        refused(b"n_views", n=n)
    refused(b"aligned", views=V + 4)
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"workspace", ws=WS + 4)
    # more views than the workspace was sized for
    assert _lib.gs_view_overlap_workspace_bytes(H, W, 2, 64) > ws_bytes
    refused(b"workspace", n=64)


def test_view_rows_are_validated_by_their_owner():
    """The rows of views_dev cannot be checked by gs_view_overlap; gs_view_overlap_check_view is what the table's owner calls
    per row (gs_slam.view_row), and the border is held against the smallest keyframe."""
    from gaussian import _lib

    import gs_slam

    def refused(word, view, border=0):
        assert _lib.gs_view_overlap_check_view(C.byref(view) if view is not None else None, border) == GS_E_INVALID
        msg = _lib.gs_last_error()
        assert b"gs_view_overlap_check_view" in msg or b"overlap_check" in msg, msg
        assert word in msg, msg

    assert _lib.gs_view_overlap_check_view(C.byref(_cam()), 0) == 0
    assert _lib.gs_view_overlap_check_view(C.byref(_cam()), H // 2 - 1) == 0
    refused(b"null", None)
    refused(b"size", _cam(width=0))
    refused(b"size", _cam(height=-1))
    refused(b"focal", _cam(focal_x=0.0))
    refused(b"focal", _cam(focal_y=float("nan")))
    refused(b"border", _cam(), border=-1)
    refused(b"border", _cam(), border=H // 2)  # 2 border >= the view's height
    refused(b"border", _cam(width=40), border=20)
    cam = R.case(37, 53, 1, 3)["views"][2]
    row = gs_slam.view_row(cam)
    assert row.dtype == np.float32 and row.tobytes() == R.table_rows([cam])[0].tobytes()
    bad = R._camera(53, 37, -1.0, 40.0, np.eye(3), np.zeros(3))
    with pytest.raises(RuntimeError, match="focal"):
        gs_slam.view_row(bad)


# ------------------------------------------------------------------------------------------ the restatements on the cases
@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.cases() + list(R.GROUP_EDGE_CASES) + list(R.LONG_CASES))
def test_restatements_agree_on_the_cases(Hc, Wc, stride, n_views):
    """A condition on the INPUTS of the GPU tier: float32 and float64 counts differ by at most the undecidable count per view,
    and no view has more undecidable points than 0.1 % of the measured ones (the seeds are chosen for that).  With the cases of
    tests/test_gpu_slam_regimes.py: the view-group edges on the smallest shape, and the multi-chunk shapes (worst view there:
    35 undecidable points of 472,498 measured ones)."""
    k = R.case(Hc, Wc, stride, n_views)
    for border in (0, 4):
        ref = R.reference(Hc, Wc, stride, n_views, border)
        c32, c64, per_view = ref["c32"], ref["c64"], ref["und_per_view"]
        measured = int(c32[n_views])
        assert measured == int(c64[n_views]) > 0.8 * len(R.lattice(Hc, Wc, stride)[0])
        assert (np.abs(c32[:n_views] - c64[:n_views]) <= per_view).all()
        assert abs(int(c32[n_views + 1]) - int(c64[n_views + 1])) <= ref["und_any"]
        assert per_view.max() <= 1e-3 * measured, (border, int(per_view.max()), measured)
        assert c32[0] == R.own_view_count(k["z"], stride, border)


def test_plan_restatement_is_the_librarys():
    """overlap_ref.plan against the one thing the library tells of its launch plan without a device: a workspace row of
    n_views + 2 uint32 per workgroup.  The old and the new shapes, 1080p at strides 1 and 2, and the boundary itself:
    OVL_MAX_BLOCKS * 256 = 524,288 lattice pixels are the most that one chunk per workgroup covers."""
    from gaussian import _lib

    assert R.plan(725, 724, 1) == (524_900, 2_051, 2, 1_026) and R.plan(1449, 1450, 2) == (524_900, 2_051, 2, 1_026)
    assert R.plan(1025, 1024, 1) == (1_049_600, 4_100, 3, 1_367)
    assert R.plan(1080, 1920, 1) == (2_073_600, 8_100, 4, 2_025) and R.plan(1080, 1920, 2) == (518_400, 2_025, 1, 2_025)
    assert R.plan(512, 1024, 1) == (524_288, 2_048, 1, 2_048) and R.plan(1024, 2048, 2) == (524_288, 2_048, 1, 2_048)
    assert R.plan(37, 53, 1) == (1_961, 8, 1, 8) and R.plan(1, 1, 3) == (0, 0, 1, 0)  # (1 x 1 at stride 3: offset 1, no lattice)
    shapes = list(R.SHAPES) + list(R.LONG_SHAPES) + [(1080, 1920, 1), (1080, 1920, 2), (512, 1024, 1), (1024, 2048, 2),
                                                       (512, 1025, 1), (1, 524_289, 1), (1, 1, 3), (2160, 3840, 1)]
    for Hc, Wc, stride in shapes:
        L, chunks, per, nblk = R.plan(Hc, Wc, stride)
        assert L == len(R.lattice(Hc, Wc, stride)[0]) and chunks == -(-L // 256)
        assert (per == 1) == (L <= 524_288) and nblk <= 2048 and nblk * per >= chunks
        assert L == 0 or (nblk - 1) * per < chunks  # the last workgroup has a chunk of its own
        for n in (1, 7, 65, 256):
            want = (4 * max(nblk, 1) * (n + 2) + 255) // 256 * 256
            assert _lib.gs_view_overlap_workspace_bytes(Hc, Wc, stride, n) == want, (Hc, Wc, stride, n)


def test_band_maps_hold_the_three_skip_situations():
    """The inputs of the no-measurement skip (tests/test_gpu_slam_regimes.py): in every multi-chunk shape's band map there is a
    workgroup whose first chunk is blank and a later one measured, one whose first chunk is measured and a later one blank,
    and one that is blank altogether -- and range_map alone has no blank chunk at all."""
    for Hc, Wc, stride in R.LONG_SHAPES:
        first_blank, later_blank, all_blank = R.skip_situations(R.band_case(Hc, Wc, stride, 7)["z"], stride)
        assert len(first_blank) and len(later_blank) and len(all_blank), (Hc, Wc, stride)
        assert R.chunk_measured(R.case(Hc, Wc, stride, 7)["z"], stride).all()


@pytest.mark.parametrize("Hc,Wc,stride", R.SHAPES)
def test_closed_form_views(Hc, Wc, stride):
    k = R.case(Hc, Wc, stride, 65)
    z = k["z"]
    n_lattice = len(R.lattice(Hc, Wc, stride)[0])
    if (Hc, Wc, stride) == (37, 53, 1):
        assert n_lattice == 1961 and R.origin(53) == 5 - 32 and R.origin(37) == 5 - 24  # the crop: left = top = 5
    for border in (0, 4):
        c = R.counts_f32(z, k["cam"], k["views"], stride, k["near"], border)
        assert c[0] == R.own_view_count(z, stride, border)  # its own camera: every point falls back on its pixel centre
        assert c[1] == 0  # turned 180 degrees about y
        assert c[65] == R.own_view_count(z, stride, 0) < n_lattice  # measured: about 10 % carry no measurement
        assert 0 < c[3] < c[65] and 0 < c[4] < c[65] and 0 < c[5] < c[65]  # sideways, yawed, forward: partial
    assert R.own_view_count(z, stride, 4) < R.own_view_count(z, stride, 0)
    # forward: the points it loses are behind `near`, not outside the image
    _, _, p = R.points(z, k["cam"], stride)
    qz, _ = R._view_terms(p, k["views"][5], 0, np.float32)
    assert 0 < int((qz <= np.float32(k["near"])).sum()) < len(qz)


# ------------------------------------------------------------------------------- the per-point header, compiled for the host
_MAIN = r"""
#include <cstdio>
#include <vector>
#include "overlap_point.h"
int main() {
    int32_t hdr[3];  // n_views, n_points, border
    float near;
    gs_seed_camera cam;
    if (fread(hdr, 4, 3, stdin) != 3 || fread(&near, 4, 1, stdin) != 1 || fread(&cam, 64, 1, stdin) != 1) return 2;
    std::vector<gs_seed_camera> views(hdr[0]);
    if (fread(views.data(), 64, hdr[0], stdin) != (size_t)hdr[0]) return 2;
    for (int i = 0; i < hdr[1]; ++i) {
        int32_t xy[2];
        float z, p[3] = {0.f, 0.f, 0.f};
        if (fread(xy, 4, 2, stdin) != 2 || fread(&z, 4, 1, stdin) != 1) return 2;
        const bool m = gs_overlap_measured(z);
        if (m) gs_overlap_point(cam, xy[0], xy[1], z, p);
        for (int k = 0; k < hdr[0]; ++k) putchar(m && gs_overlap_seen(p, views[k], near, hdr[2]) ? '1' : '0');
        putchar('\n');
    }
    return 0;
}
"""


def test_point_header_compiled_for_the_host_decides_like_the_restatement(tmp_path):
    """csrc/overlap_point.h is the kernel's own text; compiled for the host (no FMA contraction, IEEE division and square
    root) it reproduces the float32 restatement's decision for every lattice pixel and view of one case, unmeasured pixels
    included."""
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "main.cpp", tmp_path / "overlap_host"
    src.write_text(_MAIN)
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    Hc, Wc, stride, n_views = 37, 53, 1, 65
    k = R.case(Hc, Wc, stride, n_views)
    border = 4
    ys, xs = R.lattice(Hc, Wc, stride)
    blob = struct.pack("<iiif", n_views, len(ys), border, k["near"]) + R.table_rows([k["cam"]]).tobytes()
    blob += R.table_rows(k["views"]).tobytes()
    pts = np.zeros(len(ys), np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<f4")]))
    pts["x"], pts["y"], pts["z"] = xs, ys, k["z"][ys, xs]
    out = subprocess.run([str(exe)], input=blob + pts.tobytes(), stdout=subprocess.PIPE, check=True).stdout.decode().split()
    got = np.array([[ch == "1" for ch in line] for line in out])
    assert got.shape == (len(ys), n_views)
    mys, mxs, _ = R.measured_lattice(k["z"], stride)
    want = np.zeros((Hc, Wc, n_views), bool)
    want[mys, mxs] = R.seen_f32(k["z"], k["cam"], k["views"], stride, k["near"], border).T
    assert np.array_equal(got, want[ys, xs])
    assert got.any() and not got.all()


# ------------------------------------------------------------------------------------------------------ the keyframe rules
def test_select_keyframes():
    from gs_slam import select_keyframes

    assert select_keyframes([50, 90, 70, 10], 100, 2, 0.2) == [1, 2]
    assert select_keyframes([50, 90, 70, 10], 100, 9, 0.2) == [1, 2, 0]  # k larger than the set; view 3 is below min_share
    assert select_keyframes([50, 90, 70, 10], 100, 9, 0.0) == [1, 2, 0, 3]
    assert select_keyframes([70, 90, 70, 90, 70], 100, 4, 0.1) == [3, 1, 4, 2]  # ties: the more recent keyframe first
    assert select_keyframes([10, 20], 100, 2, 0.2) == [1]  # count >= min_share x measured: the bound itself counts
    assert select_keyframes([10, 19], 100, 2, 0.2) == []
    assert select_keyframes([50, 90], 100, 0, 0.1) == [] and select_keyframes([], 100, 3, 0.1) == []
    assert select_keyframes(np.array([5, 5, 5], np.int64), 5, 2, 1.0) == [2, 1]
    assert select_keyframes([0, 0], 0, 2, 0.5) == [1, 0]  # nothing measured: every view meets the (empty) bound
    assert all(type(i) is int for i in select_keyframes(np.array([3, 4]), 4, 2, 0.5))


def test_is_keyframe():
    from gs_slam import is_keyframe

    assert is_keyframe(89, 100, 1, 0.9, 5) and not is_keyframe(90, 100, 1, 0.9, 5)  # count < overlap_min x measured
    assert is_keyframe(100, 100, 5, 0.9, 5) and not is_keyframe(100, 100, 4, 0.9, 5)  # the forced interval
    assert not is_keyframe(0, 100, 1, 0.0, 1000)  # overlap_min 0: never by overlap
    assert is_keyframe(0, 0, 3, 0.0, 3) and not is_keyframe(0, 0, 2, 0.5, 3)  # nothing measured: 0 < 0 is false
    assert type(is_keyframe(np.int64(1), np.int64(2), 1, 0.9, 5)) is bool


def test_slam_options_name_their_sources():
    import gs_seed
    import gs_slam
    from gs_track import TrackOptions

    o = gs_slam.SlamOptions()
    assert o.track == TrackOptions() and o.seed == gs_seed.DEFAULTS and o.seed is not gs_seed.DEFAULTS
    assert (o.train.n_iters_warmup, o.train.depth_weight) == (5, 0.2)  # tests/test_gpu_seed.py::_trainer
    assert [f for f in gs_slam.SlamFrame.__dataclass_fields__][:8] == ["rot", "tran", "tracked", "keyframe", "overlap",
                                                                       "window", "added", "map_losses"]
    for word in ("test_gpu_seed", "n_iters", "gs_seed.DEFAULTS"):
        assert word in gs_slam.SlamOptions.__doc__
    with pytest.raises(RuntimeError):  # HIP kernels: no CPU fallback
        gs_slam.Slam(R.case(37, 53, 1, 1)["cam"], device="cpu")
    with pytest.raises(ValueError):
        gs_slam.KeyframeSet(capacity=257, device="cpu")


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


# (VGPRs, SGPRs, LDS bytes) as the build reports them.  The count kernel: three registers of world
# point, four of lane-distributed counts, a view's row in sixteen SGPRs; LDS = 4 waves x 258 uint32.  Eight waves per SIMD
# need <= 64 VGPRs and <= 80 SGPRs.  The finalize kernel: 4 waves x 64 int64 of LDS.
OVERLAP_KERNELS = {"overlap_count_kernel": (32, 80, 4128), "overlap_finalize_kernel": (16, 32, 2048)}


@pytest.mark.parametrize("part", sorted(OVERLAP_KERNELS))
def test_overlap_kernels_resources(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    vgprs, sgprs, lds = OVERLAP_KERNELS[part]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".sgpr_count"] <= sgprs, (k[".name"], k[".sgpr_count"])
    assert k[".group_segment_fixed_size"] == lds, (k[".name"], k[".group_segment_fixed_size"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch
