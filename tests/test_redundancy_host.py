"""CPU tier of the redundancy histogram and of keyframe eviction's host logic (include/gs_abi.h: gs_view_redundancy,
gs_view_redundancy_pp, gs_view_redundancy_workspace_bytes; csrc/redundancy.hip; gs_slam.select_eviction, SlamOptions): the
symbols and bindings, the workspace size query and through it the launch plan csrc/redundancy.hip restates, every refusal on
fake pointers (each comes before anything is enqueued), the eviction rule on hand-made histograms, the options' ranges, the
restatement of tests/redundancy_ref.py against overlap_ref's counts, and the resources of the three kernels read from the built
code object.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import overlap_ref as R
import redundancy_ref as RR

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

    for name in ("gs_view_redundancy_workspace_bytes", "gs_view_redundancy", "gs_view_redundancy_pp"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_view_redundancy_workspace_bytes(", "int gs_view_redundancy(", "int gs_view_redundancy_pp(",
                 "#define GS_REDUNDANCY_BINS 8"):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    assert _lib.GS_REDUNDANCY_BINS == 8
    import gs_build
    import gs_slam

    assert gs_build.SOURCES["redundancy.hip"] == gs_build.SOURCES["overlap.hip"]  # the same decisions need the same flags
    assert "-ffp-contract=off" in gs_build.SOURCES["redundancy.hip"]
    assert gs_slam.GS_REDUNDANCY_BINS == 8 and callable(gs_slam.view_redundancy)


SHAPES = list(R.SHAPES) + list(R.LONG_SHAPES) + [(480, 640, 2), (1080, 1920, 1), (1080, 1920, 2), (512, 1024, 1),
                                                 (512, 1025, 1), (1, 524_289, 1), (1, 1, 3), (2160, 3840, 1)]


def test_workspace_size_query_and_the_restated_plan():
    """One row of nine uint32 per workgroup of the count kernel, 256-aligned: the workgroups are those of overlap_ref.plan,
    which tests/test_overlap_host.py holds against csrc/overlap.hip's own plan -- so the two restatements of the plan in the
    library equal each other on every shape here, the multi-chunk ones and the threshold itself (524,288 lattice pixels)."""
    from gaussian import _lib

    q = _lib.gs_view_redundancy_workspace_bytes
    for bad in ((-1, 64, 1), (0, 64, 1), (48, 0, 1), (48, -2, 1), (48, 64, 0), (48, 64, -1)):
        assert q(*bad) == 0
    for Hc, Wc, stride in SHAPES:
        _, _, _, nblk = R.plan(Hc, Wc, stride)
        got = q(Hc, Wc, stride)
        assert got % 256 == 0 and got >= max(nblk, 1) * 9 * 4
        assert got == (max(nblk, 1) * 9 * 4 + 255) // 256 * 256, (Hc, Wc, stride)
        # the same workgroups as the overlap count: its row is n_views + 2 = 9 words with seven views
        assert got == _lib.gs_view_overlap_workspace_bytes(Hc, Wc, stride, 7)
    assert q(725, 724, 1) == (1_026 * 36 + 255) // 256 * 256 and q(1025, 1024, 1) == (1_367 * 36 + 255) // 256 * 256
    assert q(37, 53, 1) == 512  # eight workgroups, 288 bytes


def test_redundancy_rejects_bad_arguments_before_any_launch():
    """Mirror of test_overlap_rejects_bad_arguments_before_any_launch: fake device pointers throughout -- had anything been
    enqueued, the process would not survive it -- and the additional refusals: self_index and a misaligned hist_dev."""
    from gaussian import _lib

    n_views = 5
    ws_bytes = _lib.gs_view_redundancy_workspace_bytes(H, W, 2)
    Z, V, HIST, WS, VPP = (FAKE + i * (1 << 24) for i in range(5))

    def call(rng=Z, cam="default", views=V, n=n_views, self_index=2, opts="default", hist=HIST, ws=WS, nbytes=ws_bytes):
        o = _opts() if opts == "default" else opts
        c = _cam() if cam == "default" else cam
        return _lib.gs_view_redundancy(rng, C.byref(c) if c is not None else None, views, n, self_index,
                                       C.byref(o) if o is not None else None, hist, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_view_redundancy" in msg or b"redundancy_check" in msg, msg
        assert word in msg, (kw, msg)

    for kw in ("rng", "cam", "views", "opts", "hist"):
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
        refused(b"n_views", n=n, self_index=-1)
    for s in (-2, -100, n_views, n_views + 1, 1 << 20):
        refused(b"self_index", self_index=s)
    refused(b"self_index", n=1, self_index=1)
    refused(b"aligned", views=V + 4)
    refused(b"hist_dev", hist=HIST + 4)
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"workspace", ws=WS + 4)
    # a larger image than the workspace was sized for
    assert _lib.gs_view_redundancy_workspace_bytes(4 * H, 4 * W, 2) > ws_bytes
    refused(b"workspace", cam=_cam(width=4 * W, height=4 * H))

    # the variant with offsets: its own refusals, and the shared ones through it
    def call_pp(cam, vpp=VPP, self_index=2, hist=HIST):
        o = _opts()
        return _lib.gs_view_redundancy_pp(Z, C.byref(cam) if cam is not None else None, V, vpp, n_views, self_index,
                                          C.byref(o), hist, WS, ws_bytes, None)

    def cam_pp(dx=1.5, dy=-2.0):
        c = _lib.GsSeedCameraPP()
        c.cam, c.pp_dx, c.pp_dy = _cam(), dx, dy
        return c

    for args, word in (((None,), b"null"), ((cam_pp(float("nan")),), b"finite"), ((cam_pp(0.0, float("inf")),), b"finite"),
                       ((cam_pp(), VPP + 4), b"aligned"), ((cam_pp(), VPP, n_views), b"self_index"),
                       ((cam_pp(), None, -2), b"self_index"), ((cam_pp(), VPP, 2, HIST + 4), b"hist_dev")):
        assert call_pp(*args) == GS_E_INVALID, word
        msg = _lib.gs_last_error()
        assert b"gs_view_redundancy" in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------------- the eviction rule
def _hists(rows):
    return np.array(rows, np.int64)


def test_select_eviction():
    from gs_slam import select_eviction

    #           bins 0 .. 7                      measured
    h = _hists([[0, 0, 0, 100, 0, 0, 0, 0, 100],   # 0: everything seen by three others
                [50, 0, 0, 50, 0, 0, 0, 0, 100],   # 1: half
                [10, 0, 0, 0, 90, 0, 0, 0, 100],   # 2: 90 %
                [0, 0, 0, 0, 0, 0, 0, 100, 100]])  # 3: everything seen by seven or more
    assert select_eviction(h, 3, ()) == 0                      # rows 0 and 3 both score 1: the lower position
    assert select_eviction(h, 3, (0,)) == 3
    assert select_eviction(h, 3, (0, 3)) == 2                  # protected rows are never chosen
    assert select_eviction(h, 3, (0, 2, 3)) == 1
    assert select_eviction(h, 3, (0, 1, 2, 3)) is None         # all rows protected
    assert select_eviction(h, 3, range(4)) is None and select_eviction(h[:0], 3, ()) is None
    assert select_eviction(h, 4, ()) == 3                      # seen_by 4: row 0 scores 0, row 2 0.9, row 3 1
    assert select_eviction(h, 4, (3,)) == 2
    assert select_eviction(h, 7, ()) == 3                      # seen_by 7 reads bin 7 only
    assert select_eviction(h, 7, (3,)) == 0                    # ... rows 0, 1, 2 all score 0: the lowest position
    six = _hists([[0, 0, 0, 0, 0, 0, 9, 0, 10], [0, 0, 0, 0, 0, 0, 0, 8, 10]])
    assert select_eviction(six, 7, ()) == 1 and select_eviction(six, 6, ()) == 0  # bin 6 counts for 6, not for 7
    # seen_by 1: everything but bin 0
    one = _hists([[5, 1, 1, 1, 1, 1, 0, 0, 10], [4, 0, 0, 0, 0, 0, 0, 6, 10]])
    assert select_eviction(one, 1, ()) == 1
    # a row that measured nothing scores 1
    empty = _hists([[1, 0, 0, 98, 0, 0, 0, 0, 99], [0] * 9, [0, 0, 0, 7, 0, 0, 0, 0, 7]])
    assert select_eviction(empty, 3, (0,)) == 1                # 1 against 7/7: a tie, the lower position
    assert select_eviction(empty, 3, (0, 1)) == 2 and select_eviction(empty, 3, ()) == 1
    # exact fractions: 2/3 against 4/6 is a tie (in floating point 2/3 == 4/6 too, but 1/3 + 1/3 style sums need not be)
    tie = _hists([[9, 0, 0, 0, 0, 0, 0, 0, 9], [1, 0, 0, 2, 0, 0, 0, 0, 3], [2, 0, 0, 1, 2, 1, 0, 0, 6]])
    assert select_eviction(tie, 3, ()) == 1 and select_eviction(tie, 3, (1,)) == 2
    assert select_eviction(tie[::-1], 3, ()) == 0              # the 4/6 row first: it wins the tie by position
    # ... where floating point would not see one: (2^53 + 1) / 2^54 against 1/2 + a fraction that rounds away
    big = 1 << 54
    close = np.array([[big // 2 - 1, 0, 0, big // 2 + 1, 0, 0, 0, 0, big], [big // 2, 0, 0, big // 2, 0, 0, 0, 0, big]], object)
    assert float(big // 2 + 1) / float(big) == 0.5             # (the float score cannot tell them apart)
    assert select_eviction(close, 3, ()) == 0 and select_eviction(close[::-1], 3, ()) == 1
    for got in (select_eviction(h, 3, ()), select_eviction(np.asarray(h, np.int64), 3, (np.int64(0),))):
        assert type(got) is int
    for bad in (0, 8, -1):
        with pytest.raises(ValueError):
            select_eviction(h, bad, ())


def test_slam_options_eviction():
    import gs_slam

    o = gs_slam.SlamOptions()
    assert (o.max_keyframes, o.evict_seen_by, o.evict_stride) == (0, 3, None)
    cam = R.case(37, 53, 1, 1)["cam"]
    # refused before the device is asked for: "cpu" would raise RuntimeError (no CPU fallback) if the check came later
    for mk in (1, 2, 257, -1):
        with pytest.raises(ValueError, match="max_keyframes"):
            gs_slam.Slam(cam, gs_slam.SlamOptions(max_keyframes=mk), device="cpu")
    for sb in (0, 8):
        with pytest.raises(ValueError, match="evict_seen_by"):
            gs_slam.Slam(cam, gs_slam.SlamOptions(max_keyframes=4, evict_seen_by=sb), device="cpu")
        with pytest.raises(ValueError, match="evict_seen_by"):
            gs_slam.Slam(cam, gs_slam.SlamOptions(evict_seen_by=sb), device="cpu")
    with pytest.raises(ValueError, match="evict_stride"):
        gs_slam.Slam(cam, gs_slam.SlamOptions(max_keyframes=4, evict_stride=0), device="cpu")
    for mk in (0, 3, 256):  # valid: the refusal is the device's
        with pytest.raises(RuntimeError, match="HIP"):
            gs_slam.Slam(cam, gs_slam.SlamOptions(max_keyframes=mk), device="cpu")
    fields = [f for f in gs_slam.SlamFrame.__dataclass_fields__]
    assert fields[:8] == ["rot", "tran", "tracked", "keyframe", "overlap", "window", "added", "map_losses"]
    # behind every field older tests construct by position, in front of the two that tests/test_gate_map_host.py pins last
    assert fields[-2:] == ["gated", "icp"] and 8 <= fields.index("evicted") < fields.index("window_ids") < fields.index("gated")
    assert list(gs_slam.SlamOptions.__dataclass_fields__)[-5:] == ["max_keyframes", "evict_seen_by", "evict_stride", "gate_map",
                                                                    "icp"]
    f = gs_slam.SlamFrame(rot=np.eye(3), tran=np.zeros(3), tracked=None, keyframe=False, overlap=None)
    assert f.evicted is None and f.window_ids == []
    for word in ("ORB-SLAM", "evidence"):
        assert word in open(gs_slam.__file__).read()
    assert "there is no eviction" not in gs_slam.__doc__


# ------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("Hc,Wc,stride", R.SHAPES)
def test_reference_against_the_overlap_restatement(Hc, Wc, stride):
    """hist_f32 on the three-view cases: the bins sum to the point count, and -- no point can be seen by more than two other
    views, so bin 7 is empty and no count is clamped -- sum(b hist[b]) is the sum of counts_f32's per-view entries without
    row self_index.  On the larger cases: the bins still sum, and the clamp is what separates the two sums."""
    k = R.case(Hc, Wc, stride, 3)
    for border in (0, 2):
        counts = R.counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], border)
        for self_index in (-1, 0, 1, 2):
            h = RR.hist_f32(k["z"], k["cam"], k["views"], self_index, stride, k["near"], border)
            assert h.dtype == np.int64 and h.shape == (9,) and h[:8].sum() == h[8] == counts[3] > 0
            assert h[7] == 0 and h[3:8].sum() == 0
            others = np.delete(counts[:3], self_index) if self_index >= 0 else counts[:3]
            assert (np.arange(8) * h[:8]).sum() == others.sum()
        assert RR.hist_f32(k["z"], k["cam"], k["views"], -1, stride, k["near"], border)[0] == counts[4]  # seen by nobody
    k = R.case(Hc, Wc, stride, 65)
    seen = R.seen_f32(k["z"], k["cam"], k["views"], stride, k["near"], 0)
    for self_index in (-1, 0, 63, 64):
        h = RR.hist_f32(k["z"], k["cam"], k["views"], self_index, stride, k["near"], 0)
        c = (np.delete(seen, self_index, 0) if self_index >= 0 else seen).sum(0)
        assert h[:8].sum() == h[8] == seen.shape[1] and h[7] == (c >= 7).sum() > 0
        assert (np.arange(8) * h[:8]).sum() == np.minimum(c, 7).sum() < c.sum()
    one = R.case(Hc, Wc, stride, 1)
    h = RR.hist_f32(one["z"], one["cam"], one["views"], 0, stride, one["near"], 0)
    assert h[0] == h[8] > 0 and h[1:8].sum() == 0  # its own row left out of a table of one: every point in bin 0


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


# (VGPRs, SGPRs, LDS bytes) bounds; what the build reports is in DESIGN.md section 3.15.  The count kernels: three registers of
# world point and ONE counter per lane, a view's row in sixteen SGPRs, the nine bins wave-uniform; eight waves per SIMD -- the
# occupancy overlap_count_kernel is held to -- need <= 64 VGPRs (and <= 102 SGPRs, the architectural limit of a wave);
# LDS = 4 waves x 9 uint32, nothing added for the ballots.  The finalize kernel -- one workgroup, nine int64 sums a thread
# (18 registers) and the nine words of a row in flight: held to the same 64 -- has 4 waves x 9 int64 of LDS.
REDUNDANCY_KERNELS = {"redundancy_count_kernel": (64, 102, 4 * 9 * 4), "redundancy_count_pp_kernel": (64, 102, 4 * 9 * 4),
                      "redundancy_finalize_kernel": (64, 32, 4 * 9 * 8)}


@pytest.mark.parametrize("part", sorted(REDUNDANCY_KERNELS))
def test_redundancy_kernels_resources(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    vgprs, sgprs, lds = REDUNDANCY_KERNELS[part]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".sgpr_count"] <= sgprs, (k[".name"], k[".sgpr_count"])
    assert k[".group_segment_fixed_size"] == lds, (k[".name"], k[".group_segment_fixed_size"])
    assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch


def test_the_new_kernels_hide_from_the_overlap_resource_test(kernels):
    """tests/test_overlap_host.py finds its kernels by substring and wants exactly one hit each."""
    for part in ("overlap_count_kernel", "overlap_finalize_kernel"):
        assert not [k for k in kernels if part in k and "redundancy" in k]
    assert len([k for k in kernels if "redundancy_" in k]) == 3
