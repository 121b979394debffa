"""GPU: the kernels added for RGB-D SLAM -- the covisibility count (csrc/overlap.hip), the median-gated tracking loss
(csrc/track_gate.hip) and the per-Gaussian contributions (csrc/contrib.hip) -- beyond the input sizes at which each of them
takes another code path: a workgroup that runs over several chunks, a capped chunk count, a grid that strides over its work
list.  tests/test_gpu_step_regimes.py does the same for the kernels of the training step.  Every shape below is the smallest
that crosses its threshold; the thresholds are constants of the kernels and are restated here beside the source line they come
from: whoever moves one moves the test.

The references are the NumPy restatements of tests/overlap_ref.py, np.sort and gs_loss_track (through the helpers of
tests/test_gpu_track_gate.py), the library's own backward, render_aux's alpha map and tests/contrib_ref.py; every bound is the
one the existing test of the same kernel carries.  Lines that start with REGIME carry the worst error / tolerance of each
comparison and the undecidable counts (profiles/slam_kernel_regimes.txt records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import overlap_ref as R
import pp_testutil as P
from contrib_ref import composite
from gs_geometry import principal_point_offset
from gs_scene import Scene, make_camera
from gs_testutil import grad_close, to_torch
from test_gpu_contrib import B, W_MIN
from test_gpu_pp import OFF_A, _overlap_views
from test_gpu_track_gate import CW, DW, _check_contract, _crafted_run, _run_gated, _run_plain
from track_gate_ref import crafted_inputs
from track_ref import ALPHA_MIN, loss_inputs, measured

pytestmark = pytest.mark.gpu

# overlap.hip: `constexpr int OVL_BLOCK = 256` lattice pixels to a chunk; `constexpr int OVL_MAX_BLOCKS = 2048` workgroups,
# `G.chunks_per_block = chunks > OVL_MAX_BLOCKS ? gs_div_up(chunks, OVL_MAX_BLOCKS) : 1` (overlap_ref.plan restates the plan)
OVL_BLOCK, OVL_MAX_BLOCKS = 256, 2048
OVL_ONE_CHUNK = OVL_BLOCK * OVL_MAX_BLOCKS  # 524,288 lattice pixels: the most that one chunk per workgroup covers
# overlap_count_body.inc: `const int kend = min(64, n_views - 64 * g)` -- views are counted 64 to a register
OVL_GROUP = 64

# track_gate.hip: `TG_BLOCK = 256, TG_PER_BLOCK = TG_BLOCK * 4` pixels to a chunk ...
TG_PER_BLOCK = 1024
# ... `TG_RESIDUAL_BLOCKS = 512, TG_RESIDUAL_MAX_CHUNKS = 8, TG_DIGIT_BLOCKS = 128`; gs_loss_track_gated:
# `rchunks = gs_div_up(nchunks, TG_RESIDUAL_BLOCKS); if (rchunks > TG_RESIDUAL_MAX_CHUNKS) rchunks = TG_RESIDUAL_MAX_CHUNKS;`
# `dchunks = gs_div_up(nchunks, TG_DIGIT_BLOCKS)`, `rblocks = gs_div_up(nchunks, rchunks)`, `dblocks = gs_div_up(nchunks, dchunks)`
TG_RESIDUAL_BLOCKS, TG_RESIDUAL_MAX_CHUNKS, TG_DIGIT_BLOCKS = 512, 8, 128
TG_CLAMP_FROM = TG_PER_BLOCK * TG_RESIDUAL_BLOCKS * TG_RESIDUAL_MAX_CHUNKS  # 4,194,304 pixels: beyond it rchunks is clamped

# contrib.hip, gs_stage_contrib: `bwd_frame_grid` (raster_bwd_common.h) waves, at most GS_BWD_GRID_CAP of them, `kb += gridDim.x` over the work list
CONTRIB_GRID_CAP = 40960
# raster_bwd.hip, bucket_scan_kernel: the work list is the exclusive scan over the tiles of ceil(nproc / 64) buckets
GS_BUCKET = 64


def report(what, **figures):
    print("REGIME", what + ":", ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


def div_up(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ A. overlap
def _overlap_tensors(gpu, k, views=None):
    return torch.from_numpy(k["z"]).to(gpu), torch.from_numpy(R.table_rows(views or k["views"])).to(gpu)


def _assert_crosses(Hc, Wc, stride):
    L, chunks, per, nblk = R.plan(Hc, Wc, stride)
    assert L > OVL_ONE_CHUNK and per > 1 and nblk <= OVL_MAX_BLOCKS
    assert nblk * per > chunks  # the last workgroup's run ends at the `break`
    return L, chunks, per, nblk


@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.LONG_CASES)
def test_overlap_runs_of_several_chunks(gpu, Hc, Wc, stride, n_views):
    """Two and three chunks per workgroup, the ragged last workgroup, one view group and two: all n_views + 2 entries equal
    the float32 restatement, lie inside the float64 band, and the frame's own camera sees what the closed form says --
    test_counts_equal_the_float32_restatement at the multi-chunk shapes."""
    from gs_slam import view_overlap

    L, chunks, per, nblk = _assert_crosses(Hc, Wc, stride)
    k = R.case(Hc, Wc, stride, n_views)
    z, table = _overlap_tensors(gpu, k)
    for border in (0, 4):
        got = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=border).cpu().numpy()
        ref = R.reference(Hc, Wc, stride, n_views, border)
        want, c64, und = ref["c32"], ref["c64"], ref["und_per_view"]
        report(f"overlap {Hc}x{Wc}/{stride} views {n_views} border {border}, {chunks} chunks {per} per workgroup {nblk} workgroups",
               differing_entries=int((got != want).sum()),
               band=float((np.abs(got[:n_views] - c64[:n_views]) / np.maximum(und, 1)).max()),
               undecidable_worst_view=int(und.max()), undecidable_any=ref["und_any"], measured=int(want[n_views]))
        assert got.dtype == np.int64 and got.shape == (n_views + 2,)
        assert np.array_equal(got, want), (border, np.nonzero(got != want)[0][:8], got[:8], want[:8])
        assert (np.abs(got[:n_views] - c64[:n_views]) <= und).all() and got[n_views] == c64[n_views]
        assert abs(int(got[n_views + 1]) - int(c64[n_views + 1])) <= ref["und_any"]
        assert got[0] == R.own_view_count(k["z"], stride, border) and got[1] == 0
        assert und.max() <= 1e-3 * want[n_views]  # (tests/test_overlap_host.py asserts it of the inputs)


def test_overlap_runs_of_several_chunks_with_offsets(gpu):
    """gs_view_overlap_pp -- the other instantiation of the same body -- at two chunks per workgroup, with the offsets of
    test_gpu_pp.test_overlap_counts_with_offsets, against pp_testutil's float32 restatement."""
    from gs_slam import view_overlap

    Hc, Wc, stride, n_views = R.LONG_CASES[0]
    _assert_crosses(Hc, Wc, stride)
    k = R.case(Hc, Wc, stride, n_views)
    cam, views = P.offset_camera(k["cam"], OFF_A), _overlap_views(k)
    z, table = _overlap_tensors(gpu, k, views)
    pp = np.array([principal_point_offset(v) for v in views], np.float32)
    assert pp.any() and principal_point_offset(cam) != (0.0, 0.0)
    table_pp = torch.from_numpy(pp).to(gpu)
    for border in (0, 4):
        got = view_overlap(z, cam, table, n_views, stride, k["near"], border, table_pp).cpu().numpy()
        want = P.overlap_counts_f32(k["z"], cam, views, stride, k["near"], border)
        report(f"overlap_pp {Hc}x{Wc}/{stride} views {n_views} border {border}", differing_entries=int((got != want).sum()))
        assert np.array_equal(got, want), (border, got, want)
        assert got[0] == R.own_view_count(k["z"], stride, border)  # its own camera and offset
        assert got[3] == 0 and 0 < got[n_views]                    # the offset alone: nothing of the frame is seen


@pytest.mark.parametrize("Hc,Wc,stride", R.LONG_SHAPES)
def test_overlap_skips_waves_without_a_measurement(gpu, Hc, Wc, stride):
    """Whole lattice rows without a measurement (0, NaN, -1 and inf): a wave whose 64 pixels are all unmeasured leaves the view
    loop out -- as the first chunk of a run, in the middle of one, and for a whole workgroup -- and the carried counts must not
    notice.  Every entry against the float32 restatement, `measured` and `seen by nobody` included."""
    from gs_slam import view_overlap

    L, chunks, per, nblk = _assert_crosses(Hc, Wc, stride)
    n_views = 7
    k = R.band_case(Hc, Wc, stride, n_views)
    first_blank, later_blank, all_blank = R.skip_situations(k["z"], stride)
    assert len(first_blank) and len(later_blank) and len(all_blank)
    z, table = _overlap_tensors(gpu, k)
    for border in (0, 4):
        got = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=border).cpu().numpy()
        want = R.counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], border)
        report(f"overlap bands {Hc}x{Wc}/{stride} border {border}, workgroups first chunk blank {first_blank[:3].tolist()} "
               f"later chunk blank {later_blank[:3].tolist()} all blank {all_blank[:3].tolist()}",
               differing_entries=int((got != want).sum()), measured=int(want[n_views]), seen_by_nobody=int(want[n_views + 1]))
        assert np.array_equal(got, want), (border, got, want)
        assert got[0] == R.own_view_count(k["z"], stride, border) and got[1] == 0
        assert 0 < got[n_views] < R.reference(Hc, Wc, stride, n_views, border)["c32"][n_views]  # fewer than without the bands
    assert got[n_views + 1] > 0  # border 4: points that no view sees, carried through the runs like the rest


def test_overlap_long_run_is_a_pure_function_of_the_inputs(gpu):
    """Two runs bitwise equal at two chunks per workgroup, one of them on a workspace and a counts_dev pre-filled with 0xFF."""
    from gaussian import _lib
    from gs_seed import seed_camera
    from gs_slam import view_overlap

    Hc, Wc, stride, n_views = R.LONG_CASES[0]
    _assert_crosses(Hc, Wc, stride)
    k = R.case(Hc, Wc, stride, n_views)
    z, table = _overlap_tensors(gpu, k)
    first = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=4)
    cam, opts = seed_camera(k["cam"]), _lib.GsOverlapOpts(stride, k["near"], 4)
    nbytes = int(_lib.gs_view_overlap_workspace_bytes(Hc, Wc, stride, n_views))
    assert nbytes == (4 * R.plan(Hc, Wc, stride)[3] * (n_views + 2) + 255) // 256 * 256
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
    counts = torch.full((n_views + 2,), -1, dtype=torch.int64, device=gpu)  # (0xFF in every byte)
    _lib.check(_lib.gs_view_overlap(z.data_ptr(), C.byref(cam), table.data_ptr(), n_views, C.byref(opts), counts.data_ptr(),
                                    ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "gs_view_overlap")
    assert torch.equal(first, counts)
    assert np.array_equal(first.cpu().numpy(), R.reference(Hc, Wc, stride, n_views, 4)["c32"])
    report(f"overlap purity {Hc}x{Wc}/{stride} views {n_views}", differing_entries=int((first != counts).sum()))


@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.GROUP_EDGE_CASES)
def test_overlap_view_group_edges(gpu, Hc, Wc, stride, n_views):
    """n_views = 64, 128, 129, 192, 193: a last group that is full, and one that holds a single view."""
    from gs_slam import view_overlap

    assert n_views % OVL_GROUP in (0, 1) and n_views >= OVL_GROUP
    k = R.case(Hc, Wc, stride, n_views)
    z, table = _overlap_tensors(gpu, k)
    for border in (0, 4):
        got = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=border).cpu().numpy()
        ref = R.reference(Hc, Wc, stride, n_views, border)
        want, c64, und = ref["c32"], ref["c64"], ref["und_per_view"]
        report(f"overlap {Hc}x{Wc}/{stride} views {n_views} border {border}", differing_entries=int((got != want).sum()),
               undecidable_worst_view=int(und.max()), undecidable_any=ref["und_any"], measured=int(want[n_views]))
        assert np.array_equal(got, want), (border, np.nonzero(got != want)[0][:8])
        assert (np.abs(got[:n_views] - c64[:n_views]) <= und).all() and got[n_views] == c64[n_views]
        assert abs(int(got[n_views + 1]) - int(c64[n_views + 1])) <= ref["und_any"]
        assert got[0] == R.own_view_count(k["z"], stride, border) and got[1] == 0
        assert got[n_views - 1] > 0  # the last view of the last group counts something


# ------------------------------------------------------------------------------------------------- B. gated tracking loss
def gate_plan(n):
    """-> (nchunks, rchunks before the clamp, rchunks, rblocks, dchunks, dblocks) as gs_loss_track_gated forms them."""
    nchunks = div_up(n, TG_PER_BLOCK)
    raw = div_up(nchunks, TG_RESIDUAL_BLOCKS)
    rchunks = min(raw, TG_RESIDUAL_MAX_CHUNKS)
    dchunks = div_up(nchunks, TG_DIGIT_BLOCKS)
    return nchunks, raw, rchunks, div_up(nchunks, rchunks), dchunks, div_up(nchunks, dchunks)


GATE_SHAPES = {(727, 723): (514, 2, 2, 257, 5, 103), (2051, 2047): (4100, 9, 8, 513, 33, 125)}


def _assert_gate_plan(H, W):
    n = H * W
    plan = gate_plan(n)
    assert plan == GATE_SHAPES[(H, W)]
    nchunks, raw, rchunks, rblocks, dchunks, dblocks = plan
    assert n % 4 == 1 and rchunks > 1 and dchunks > 1  # a tail pixel inside a multi-chunk workgroup, in both passes
    assert dblocks * dchunks > nchunks  # the last digit workgroup starts chunks that do not exist
    if n > TG_CLAMP_FROM:
        assert raw > rchunks == TG_RESIDUAL_MAX_CHUNKS and rblocks > TG_RESIDUAL_BLOCKS
        assert div_up(nchunks, raw) * rchunks < nchunks  # (a grid sized by the unclamped count would not reach the end)
    return plan


@pytest.mark.parametrize("H,W,couple", [(727, 723, True), (727, 723, False), (2051, 2047, True)])
def test_gate_tail_pixel_in_multi_chunk_workgroups(gpu, H, W, couple):
    """test_gpu_track_gate.test_selection_and_masks_are_exact, every check with its bounds, at 525,621 pixels (two chunks per
    residual workgroup, five per digit workgroup, n % 4 = 1, the last digit workgroup running past the image) and at 4,198,397
    (rchunks clamped from 9 to 8: 513 residual workgroups)."""
    from gs_train import GatedTrackLoss

    plan = _assert_gate_plan(H, W)
    x = loss_inputs(H, W, H + W)
    I, D, A, T, z = x
    scale = 0.37 / (H * W)
    t = [torch.from_numpy(a).to(gpu) for a in x]
    gl = GatedTrackLoss(H, W, ALPHA_MIN, CW, DW, 1.5, 1.5, 0.0, 0.0, couple, gpu, keep_residuals=True)
    out = _run_gated(gl, t, scale)
    out2 = _run_gated(gl, t, scale)
    for a, b in zip(out[:4], out2[:4]):
        assert torch.equal(a, b) and not torch.isnan(a).any()  # bitwise repeatable, everything written
    for a, b in zip(out[4:], out2[4:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # (the maps hold NaNs by contract)
    ref = _check_contract(out, _run_plain(H, W, t, scale, gpu), x, 1.5, 1.5, 0.0, 0.0, couple, f"gate {W}x{H} couple={couple}")
    # non-vacuity
    ra, rc = out[4].cpu().numpy(), out[5].cpu().numpy()
    with np.errstate(invalid="ignore"):
        cut_d = 1.0 - float((ra <= ref["t_d"]).sum()) / ref["n_d"]
        cut_c = 1.0 - float((rc <= ref["t_c"]).sum()) / ref["n_c"]
    assert 0.05 <= cut_d <= 0.60 and 0.05 <= cut_c <= 0.60
    # the residual maps against fp64: NaN exactly outside the sets -- a chunk no workgroup reached keeps its NaN fill
    covered, meas = A >= np.float32(ALPHA_MIN), measured(z)
    s_d = covered & meas
    wrong_d, wrong_c = np.flatnonzero(np.isnan(ra) != ~s_d), np.flatnonzero(np.isnan(rc) != ~covered)
    assert not len(wrong_d) and not len(wrong_c), \
        f"residual maps: {len(wrong_d)} depth and {len(wrong_c)} colour pixels on the wrong side of their set, the first at " \
        f"pixel {int(np.concatenate([wrong_d, wrong_c]).min())} = chunk {int(np.concatenate([wrong_d, wrong_c]).min()) // TG_PER_BLOCK}"
    e64 = D.astype(np.float64)[s_d] / A.astype(np.float64)[s_d]
    z64 = z.astype(np.float64)[s_d]
    err_a = float((np.abs(ra[s_d] - np.abs(e64 - z64)) / np.maximum(np.abs(e64), np.abs(z64))).max())
    c64 = np.abs(I.astype(np.float64) - T.astype(np.float64)).sum(axis=2)
    err_c = float(np.abs(rc[covered] - c64[covered]).max())
    # the values
    v = out[3].cpu().numpy().astype(np.float64)
    colour = scale * CW * float(c64[ref["cmask"]].sum())
    e_all = np.abs(D.astype(np.float64) / A.astype(np.float64) - np.where(meas, z, 0).astype(np.float64))
    depth = scale * DW * float(e_all[ref["dmask"]].sum())
    wants = (colour + depth, colour, depth)
    report(f"gate {H}x{W} couple={couple}, chunks/rchunks raw/rchunks/rblocks/dchunks/dblocks {plan}",
           resid_a=err_a / 1e-6, resid_c=err_c / 1e-6, values=max(abs(v[j] - wants[j]) / (1e-5 * wants[j]) for j in range(3)),
           cut_depth=cut_d, cut_colour=cut_c, n_d=ref["n_d"], n_c=ref["n_c"])
    assert err_a <= 1e-6 and err_c <= 1e-6
    for got, want in zip(v[:3], wants):
        assert want > 0 and abs(got - want) <= 1e-5 * want
    # the tail pixel itself took part: it is the last element of both maps
    assert np.isnan(ra.reshape(-1)[-1]) == (not s_d.reshape(-1)[-1]) and np.isnan(rc.reshape(-1)[-1]) == (not covered.reshape(-1)[-1])


def test_gate_crafted_tail_pixel_is_cut(gpu):
    """Every residual 1 except the last pixel's -- the tail pixel of a two-chunk residual workgroup and of a five-chunk digit
    workgroup --, which is 4: median 1, threshold 1.5, the tail pixel alone is cut, its gradients are exact zeros (its colour
    term too: coupled) and both counts are n - 1."""
    H, W = 727, 723
    _assert_gate_plan(H, W)
    n = H * W
    resid = np.ones(n, np.float32)
    resid[-1] = 4.0
    x = crafted_inputs(H, W, resid)
    (gi, gd, ga, vals, ra, rc), ref = _crafted_run(gpu, H, W, x, 1.5, tag=f"crafted tail {W}x{H}")
    assert np.array_equal(ra.reshape(-1), resid)  # exact by construction: the tail pixel's residual was stored
    assert vals[5] == 1.0 and vals[7] == n and vals[3] == n - 1 and vals[4] == n - 1
    bits = [a.reshape(n, -1).view(np.uint32) for a in (gd, ga, gi)]
    assert not bits[0][-1].any() and not bits[1][-1].any() and not bits[2][-1].any()  # +0.0
    assert np.all(gd.reshape(-1)[:-1] != 0) and np.all(gi.reshape(n, 3)[:-1].any(1))
    report(f"gate crafted tail {H}x{W}", counted_depth=int(vals[3]), counted_colour=int(vals[4]), n=n)


# ------------------------------------------------------------------------- C. the contribution pair pass beyond its grid
CW_, CH_ = 2550, 1915  # padded 2560 x 1920 (crop left 5, top 2): 160 x 120 = 19,200 tiles
BASE_PER_TILE = 6      # Gaussians centred in every tile whose rectangle is 5 x 5 tiles: interior lists of 150 = 3 buckets
PILES = (1, 42, 43, 106, 107, 400)  # small Gaussians more in the tiles the restatement composites: 151 ... 550 entries
_CONTRIB = {}


def _pad(v):
    return (v + 15) // 16 * 16


def _contrib_scene():
    """Six Gaussians near the centre of every tile with sigma 11.5 pixels -- the listing rectangle reaches 2.45 sigma = 28
    pixels, two tiles to every side --, and piles of PILES (and twice 800) small ones (sigma 1.3: listed in their own tile
    alone) in 21 tiles of the first three tile rows and 23 of the last five, whose buckets lie beyond the pair pass's grid.
    test_gpu_contrib's _Builder, vectorised: padded pixel coordinates for make_camera(W, H), isotropic, identity rotation.
    Faint: the wide ones peak at alpha <= 0.02, a pile of p at min(0.05, 5 / p) -- the optical depth of a pixel stays below
    about 4, its transmittance above 0.01: no tile stops inside its list."""
    rng = np.random.default_rng(41)
    ntx, nty = _pad(CW_) // 16, _pad(CH_) // 16
    f = 0.75 * CW_
    ty, tx = np.divmod(np.arange(ntx * nty), ntx)
    tile = [np.repeat(np.arange(ntx * nty), BASE_PER_TILE)]
    sigma = [np.full(ntx * nty * BASE_PER_TILE, 11.5)]
    peak = [np.full(ntx * nty * BASE_PER_TILE, 0.02)]
    early = [r * ntx + c for r in (0, 1, 2) for c in (0, 27, 53, 80, 106, 133, 159)]
    late = [r * ntx + c for r in (115, 116, 117, 118, 119) for c in (0, 40, 80, 120, 159)][:23]
    for j, t in enumerate(early + late):
        p = 800 if j in (10, 32) else PILES[j % len(PILES)]
        tile.append(np.full(p, t))
        sigma.append(np.full(p, 1.3))
        peak.append(np.full(p, min(0.05, 5.0 / p)))
    tile, sigma, peak = np.concatenate(tile), np.concatenate(sigma), np.concatenate(peak)
    n = len(tile)
    px = 16 * tx[tile] + 8 + rng.uniform(-2, 2, n)
    py = 16 * ty[tile] + 8 + rng.uniform(-2, 2, n)
    zc = rng.uniform(1.0, 6.0, n)
    peak = peak * rng.uniform(0.5, 1.0, n)
    s = np.maximum(sigma * zc / f - 1e-4, 1e-6)
    pos = np.stack([(px - _pad(CW_) / 2) / f * zc, (py - _pad(CH_) / 2) / f * zc, zc], 1)
    quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    scene = Scene(pos.astype(np.float32), quat.astype(np.float32), np.repeat(s[:, None], 3, 1).astype(np.float32),
                  np.log(peak / (1.0 - peak)).astype(np.float32), rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32))
    return scene, sorted(early + late), sigma < 2.0


def _tile_nproc(r):
    """int64 [T]: the Gaussians each tile of the last training forward composited (what composited_steps() adds up)."""
    from gaussian import _lib

    ptr = C.c_void_p()
    _lib.check(_lib.gs_frame_debug_tile_nproc(C.byref(r._frame), C.byref(ptr)), "gs_frame_debug_tile_nproc")
    off = ptr.value - r._ws.data_ptr()
    return r._ws[off:off + 4 * r._grid.n_tiles].view(torch.int32).to(torch.int64).cpu().numpy()


def _contrib_case(gpu):
    """The frame, rendered once as a training frame; its contributions; where each tile's buckets lie in the work list; the
    slot of every pair's row in the pass's workspace (pair_offsets[g] + the tile's index in g's rectangle)."""
    from gs_frame import FrameRenderer

    if not _CONTRIB:
        scene, pile_tiles, small = _contrib_scene()
        cam = make_camera(CW_, CH_)
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 22, training=True, bwd_rows=False)
        image, _ = r.forward(*params, cam, training=True)
        c = r.contributions(W_MIN)
        v = r.debug_views()
        ranges = v["tile_ranges"].cpu().numpy().astype(np.int64)
        ids = v["sorted_ids"].cpu().numpy().astype(np.int64)
        lists = ranges[:, 1] - ranges[:, 0]
        nproc = _tile_nproc(r)
        assert scene.n <= 200_000 and lists.max() <= 1000 and lists.min() >= 1
        assert r.stats().overflow == 0 and np.array_equal(nproc, lists) and float(image.max()) < 1.0  # no tile stops inside its list
        first = np.concatenate([[0], np.cumsum(div_up(nproc, GS_BUCKET))])  # the work-list position of a tile's first bucket
        assert CONTRIB_GRID_CAP < first[-1] < 60_000
        ntx = _pad(cam.width) // 16
        rects = r._rects().cpu().numpy().astype(np.int64) & 0xffffffff
        touched = np.where(rects[:, 2] != 0, rects[:, 3], 0)
        offs = np.cumsum(touched) - touched
        y0, x0, x1 = rects[:, 0] & 0xffff, rects[:, 1] & 0xffff, rects[:, 1] >> 16
        tile = np.repeat(np.arange(len(lists)), lists)
        assert len(tile) == len(ids) and np.array_equal(ranges[1:, 0], ranges[:-1, 1])  # the lists tile the id array in order
        slots = offs[ids] + (tile // ntx - y0[ids]) * (x1[ids] - x0[ids]) + (tile % ntx - x0[ids])
        assert len(np.unique(slots)) == len(slots) and slots.max() < int(r._frame.max_pairs)
        _CONTRIB.update(scene=scene, cam=cam, params=params, r=r, c=c, rows=c.rows.clone(), views=v, ranges=ranges, ids=ids,
                        first=first, pile_tiles=pile_tiles, small=small, tile=tile, slots=slots, touched=touched)
    return _CONTRIB


def _pair_rows(r):
    """The pass's workspace behind its 256-byte header as [max_pairs, 4] float32 (sum, max, count bits, 0), on the device."""
    base = (r._contrib_ws.data_ptr() + 255) // 256 * 256 - r._contrib_ws.data_ptr() + 256
    return r._contrib_ws[base:base + 16 * int(r._frame.max_pairs)].view(torch.float32).reshape(-1, 4)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _amax(index, values, n):
    out = np.zeros(n)
    np.maximum.at(out, index, values)
    return out


@pytest.mark.parametrize("bwd_rows", [False, True])
def test_contrib_weight_sum_beyond_the_grid_is_the_colour_gradient(gpu, bwd_rows):
    """test_weight_sum_is_the_colour_gradient_of_a_ones_image with more buckets than the pair pass has waves: the weight sum
    of every Gaussian against the library's own colour gradient of a ones image (whose kernels are held to the oracle at full
    size by test_reference_api_full_size), by grad_close, under both backward kernels."""
    from gaussian import _lib
    from gs_frame import FrameRenderer

    k = _contrib_case(gpu)
    params = k["params"]
    r = FrameRenderer(gpu, max_pairs=1 << 22, training=True, bwd_rows=bwd_rows)
    image, _ = r.forward(*params, k["cam"], training=True)
    assert float(image.max()) < 1.0
    c = r.contributions()
    g = torch.zeros_like(image)
    g[..., 0] = 1.0
    grads = r.backward(g)
    assert bool(r._frame.flags & _lib.GS_FRAME_BWD_ROWS) == bwd_rows
    buckets = r.stats().buckets
    assert buckets > CONTRIB_GRID_CAP and buckets == k["first"][-1]
    s = torch.sigmoid(params[4][:, 0].double())
    ref = (grads[4][:, 0].double() / (s * (1 - s))).cpu().numpy()
    got = c.weight_sum.cpu().numpy()
    ok, worst, where, pure = grad_close(got, ref, np.abs(ref))
    # the Gaussians with a pair in a tile whose buckets the first trip of the grid does not reach
    beyond = np.zeros(k["scene"].n, bool)
    beyond[k["ids"][k["first"][k["tile"]] >= CONTRIB_GRID_CAP]] = True
    ok_b, worst_b, where_b, _ = grad_close(got[beyond], ref[beyond], np.abs(ref[beyond]))
    report(f"contrib against the backward rows={bwd_rows}, N {k['scene'].n} pairs {len(k['ids'])} buckets {buckets}", worst=worst,
           within_rtol=pure, worst_beyond_the_grid=worst_b, gaussians_beyond_the_grid=int(beyond.sum()))
    assert beyond.sum() > 1000 and float(np.abs(ref[beyond]).max()) > 0.3
    assert ok_b, (f"Gaussian {int(np.flatnonzero(beyond)[where_b[0]])}, listed in a tile beyond the grid: weight sum "
                  f"{got[beyond][where_b[0]]!r}, from the backward {ref[beyond][where_b[0]]!r}", worst_b)
    assert ok and float(np.abs(ref).max()) > 0.3, (worst, where)
    assert np.array_equal(_bits(c.rows), _bits(k["rows"]))  # (the backward kernel choice does not reach the pass)


def test_contrib_pair_rows_beyond_the_grid_add_up_to_the_alpha_map(gpu):
    """test_pair_rows_add_up_to_the_alpha_map_per_tile over all 19,200 tiles, vectorised: the pair rows of a tile's list, read
    from the pass's zero-filled workspace at the slots the gradient rows have, against the sum of render_aux's alpha map over
    the tile's image pixels, within 256 x 5e-5."""
    from gs_frame import FrameRenderer

    k = _contrib_case(gpu)
    r, cam = k["r"], k["cam"]
    _, _, _, alpha = FrameRenderer(gpu, max_pairs=1 << 22).forward(*k["params"], cam, training=False, aux=True)
    r._contrib_ws.zero_()
    r.forward(*k["params"], cam, training=True)
    c = r.contributions()
    assert np.array_equal(_bits(c.rows), _bits(k["rows"]))  # (a zero-filled workspace: the same bytes)
    pair = _pair_rows(r)[:, 0].cpu().double().numpy()
    ntx, nty = _pad(cam.width) // 16, _pad(cam.height) // 16
    crop_top, crop_left = (_pad(cam.height) - cam.height) // 2, (_pad(cam.width) - cam.width) // 2
    padded = np.zeros((_pad(cam.height), _pad(cam.width)))
    padded[crop_top:crop_top + cam.height, crop_left:crop_left + cam.width] = alpha.cpu().double().numpy()
    want = padded.reshape(nty, 16, ntx, 16).sum((1, 3)).reshape(-1)
    got = np.bincount(k["tile"], weights=pair[k["slots"]], minlength=ntx * nty)
    err = np.abs(got - want)
    beyond = k["first"][:-1] >= CONTRIB_GRID_CAP
    report(f"contrib per tile, {ntx * nty} tiles of which {int(beyond.sum())} beyond the grid", worst=float(err.max() / (256 * 5e-5)),
           worst_beyond_the_grid=float(err[beyond].max() / (256 * 5e-5)), smallest_alpha_sum=float(want.min()))
    assert beyond.sum() > 1000 and want[beyond].min() > 10 * 256 * 5e-5  # rows left unwritten (0) would show
    t = int(err.argmax())
    assert err.max() <= 256 * 5e-5, (f"tile {t}, first bucket at work-list position {int(k['first'][t])}: sum of pair rows "
                                     f"{got[t]!r}, sum of alpha {want[t]!r}")


def test_contrib_beyond_the_grid_lies_in_the_restatements_interval(gpu):
    """test_contributions_lie_in_the_restatements_interval on the 44 pile tiles -- lists of 55 to 950 entries, 23 of them with
    every bucket at a work-list position >= 40,960 --, compacted into a frame of one tile row of their own (a pair becomes a
    Gaussian of its own, moved with its tile; the restatement's [M, 256] array would not fit for the whole frame).  Every pair
    row of those tiles (sum, maximum, count) and the finished rows of the Gaussians all of whose pairs lie in them are held to
    contrib_ref.composite at both ends of the band, with the tolerances of that test (t = 1e-4 |sum| + 1e-6 x the image
    pixels of the tiles concerned; 1e-4 |max| + 1e-6; the count inside the two ends')."""
    k = _contrib_case(gpu)
    c, cam, v, r = k["c"], k["cam"], k["views"], k["r"]
    ids, ranges, first = k["ids"], k["ranges"], k["first"]
    tiles = np.array(k["pile_tiles"])
    all_beyond = first[tiles] >= CONTRIB_GRID_CAP
    assert len(tiles) >= 40 and 2 * all_beyond.sum() >= len(tiles) and (first[tiles + 1] <= CONTRIB_GRID_CAP).sum() >= 10
    lens = ranges[tiles, 1] - ranges[tiles, 0]
    assert len(set(div_up(lens, GS_BUCKET).tolist())) >= 5 and lens.max() > 900, lens
    sel = np.concatenate([np.arange(ranges[t, 0], ranges[t, 1]) for t in tiles])
    g = ids[sel]  # the Gaussian of each compacted pair
    slot = np.repeat(np.arange(len(tiles)), lens)  # its tile in the small frame
    ntx = _pad(cam.width) // 16
    fx, fy = float(r._frame.focal_x), float(r._frame.focal_y)
    geom = v["rec_geom"].cpu().double().numpy()[g]
    cov = v["rec_cov"].cpu().double().numpy()[g]
    # pixel centres: (16 tx + lx + 0.5 - padW // 2) / fx in the frame, (16 slot + lx + 0.5 - padW' // 2) / fx in the small one
    small_w = 16 * len(tiles)
    geom[:, 0] += (16.0 * (slot - tiles[slot] % ntx) - small_w // 2 + _pad(cam.width) // 2) / fx
    geom[:, 1] += (-16.0 * (tiles[slot] // ntx) - 8 + _pad(cam.height) // 2) / fy
    small_ranges = np.stack([np.cumsum(lens) - lens, np.cumsum(lens)], 1)
    args = (np.arange(len(sel)), small_ranges, geom, cov, small_w, 16, fx, fy)
    # which of a tile's 256 pixels lie inside the cropped image of the REAL frame
    crop_top, crop_left = (_pad(cam.height) - cam.height) // 2, (_pad(cam.width) - cam.width) // 2
    lx, ly = np.arange(256) % 16, np.arange(256) // 16
    ix = 16 * (tiles % ntx)[:, None] + lx - crop_left
    iy = 16 * (tiles // ntx)[:, None] + ly - crop_top
    inside = ((ix >= 0) & (ix < cam.width) & (iy >= 0) & (iy < cam.height))[slot]
    assert not inside.all() and inside.any(1).all()  # tiles of the padded border are among them
    n = k["scene"].n
    per_g = np.bincount(g, minlength=n)
    whole = (per_g == k["touched"]) & (per_g > 0)  # every pair of the Gaussian is in a pile tile
    assert np.array_equal(whole, k["small"])  # ... the piles themselves

    def stats(stop, w_min):
        w = composite(*args, stop=stop, w_min=w_min).w.numpy() * inside
        return w.sum(1), w.max(1), (w >= w_min).sum(1)

    lo = stats(1e-4 * (1 + B), W_MIN * (1 + B))  # stops earlier, counts fewer
    hi = stats(1e-4 * (1 - B), W_MIN * (1 - B))
    # 1. the pair rows
    rows = _pair_rows(r)[torch.from_numpy(k["slots"][sel]).to(gpu)].cpu()
    got_sum, got_max = rows[:, 0].double().numpy(), rows[:, 1].double().numpy()
    got_pix = rows[:, 2].contiguous().view(torch.int32).numpy().astype(np.int64)
    pixels = inside.sum(1)
    out_sum = np.maximum((lo[0] - got_sum) / np.maximum(1e-4 * np.abs(lo[0]) + 1e-6 * pixels, 1e-30),
                         (got_sum - hi[0]) / np.maximum(1e-4 * np.abs(hi[0]) + 1e-6 * pixels, 1e-30))
    out_max = np.maximum((lo[1] - got_max) / (1e-4 * np.abs(lo[1]) + 1e-6), (got_max - hi[1]) / (1e-4 * np.abs(hi[1]) + 1e-6))
    pix_out = (got_pix < lo[2]) | (got_pix > hi[2])
    late = all_beyond[slot]
    report(f"contrib pair rows on {len(tiles)} tiles ({int(all_beyond.sum())} beyond the grid), {len(sel)} pairs ({int(late.sum())} "
           f"beyond), lists {sorted(set(lens.tolist()))}", weight_sum=float(out_sum.max()), weight_max=float(out_max.max()),
           weight_sum_beyond=float(out_sum[late].max()), weight_max_beyond=float(out_max[late].max()),
           pixels_outside=int(pix_out.sum()), rows_with_pixels=int((got_pix > 0).sum()))
    assert late.sum() >= 1000 and (got_pix[late] > 0).sum() >= 100
    j = int(out_sum.argmax())
    assert out_sum[j] <= 1.0, (f"pair {int(sel[j])} of tile {int(tiles[slot[j]])} (first bucket at work-list position "
                               f"{int(first[tiles[slot[j]]])}): sum {got_sum[j]!r} outside [{lo[0][j]!r}, {hi[0][j]!r}]", float(out_sum[j]))
    assert (out_max <= 1.0).all(), (int(sel[out_max.argmax()]), float(out_max.max()))
    assert not pix_out.any()
    # 2. the finished rows of the piles' Gaussians: one pair each
    f_sum, f_max = c.weight_sum.cpu().double().numpy(), c.weight_max.cpu().double().numpy()
    f_pix, f_views = c.pixels.cpu().long().numpy(), c.views.cpu().long().numpy()
    one = whole[g]
    assert np.array_equal(per_g[whole], np.ones(int(whole.sum()), np.int64))
    assert np.array_equal(f_sum[g[one]], got_sum[one]) and np.array_equal(f_max[g[one]], got_max[one])
    assert np.array_equal(f_pix[g[one]], got_pix[one]) and np.array_equal(f_views, (f_pix > 0).astype(np.int64))


def test_contrib_beyond_the_grid_two_calls_and_any_workspace_bytes(gpu):
    """Two calls give bitwise the same rows, from a workspace of 0xFF bytes and from a zeroed one."""
    from gs_frame import Contributions

    k = _contrib_case(gpu)
    r = k["r"]
    r.forward(*k["params"], k["cam"], training=True)
    again = r.contributions()
    assert np.array_equal(_bits(again.rows), _bits(k["rows"]))
    for fill in (0xFF, 0x00):
        r._contrib_ws.fill_(fill)
        out = Contributions(torch.full((k["scene"].n * 16,), 0xFF, dtype=torch.uint8, device=gpu).view(torch.float32)
                            .view(-1, 4), W_MIN)
        assert np.array_equal(_bits(r.contributions(out=out).rows), _bits(k["rows"])), fill
    report("contrib bitwise, workspace 0xFF and 0x00", differing_rows=0)
