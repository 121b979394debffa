"""GPU tier of the redundancy histogram (csrc/redundancy.hip through gs_slam.view_redundancy / KeyframeSet.redundancy) and of
KeyframeSet's removal: every histogram against the float32 restatement of tests/redundancy_ref.py, integer for integer -- the
shapes and view counts of the overlap tests, the row left out at both ends and on either side of the sibling kernel's register
groups, multi-chunk runs with a ragged last chunk, waves and chunks without a measurement, principal-point offsets --, against
gs_view_overlap's own counts, bitwise repeatable whatever the workspace held; and the keyframe table after a removal against a
fresh one."""
import ctypes as C

import numpy as np
import pytest
import torch

import overlap_ref as R
import pp_testutil as P
import redundancy_ref as RR

pytestmark = pytest.mark.gpu

_SEEN = {}


def _seen(k, key, border):
    """seen_f32 of a case, evaluated once per (case, border) and shared (the row left out is taken from it afterwards)."""
    key = key + (border,)
    if key not in _SEEN:
        _SEEN[key] = R.seen_f32(k["z"], k["cam"], k["views"], k["stride"], k["near"], border)
    return _SEEN[key]


def _tensors(gpu, k):
    return torch.from_numpy(k["z"]).to(gpu), torch.from_numpy(R.table_rows(k["views"])).to(gpu)


def _self_indices(n):
    return sorted({-1, 0, n - 1} | {s for s in (63, 64) if s < n})


@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.cases())
def test_hist_equals_the_float32_restatement(gpu, Hc, Wc, stride, n_views):
    from gs_slam import view_redundancy

    k = R.case(Hc, Wc, stride, n_views)
    z, table = _tensors(gpu, k)
    for border in (0, 2):
        seen = _seen(k, (Hc, Wc, stride, n_views), border)
        for s in _self_indices(n_views):
            got = view_redundancy(z, k["cam"], table, n_views, s, stride=stride, near=k["near"], border=border).cpu().numpy()
            want = RR.hist_from_seen(seen, s)
            assert got.dtype == np.int64 and got.shape == (9,)
            assert np.array_equal(got, want), (border, s, got, want)
            assert got[:8].sum() == got[8] > 0
        if n_views == 1:  # its own row left out of a table of one: every measured point in bin 0
            got = view_redundancy(z, k["cam"], table, 1, 0, stride=stride, near=k["near"], border=border).cpu().numpy()
            assert got[0] == got[8] and got[1:8].sum() == 0
    # (the restatement itself, once, through its front door)
    assert np.array_equal(RR.hist_from_seen(_seen(k, (Hc, Wc, stride, n_views), 0), n_views - 1),
                          RR.hist_f32(k["z"], k["cam"], k["views"], n_views - 1, stride, k["near"], 0))


@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.GROUP_EDGE_CASES)
def test_hist_at_the_view_group_edges(gpu, Hc, Wc, stride, n_views):
    from gs_slam import view_redundancy

    k = R.case(Hc, Wc, stride, n_views)
    z, table = _tensors(gpu, k)
    got = view_redundancy(z, k["cam"], table, n_views, n_views - 1, stride=stride, near=k["near"], border=0).cpu().numpy()
    want = RR.hist_f32(k["z"], k["cam"], k["views"], n_views - 1, stride, k["near"], 0)
    assert np.array_equal(got, want), (got, want)


LONG = (725, 724, 1, 7)
assert LONG in R.LONG_CASES


@pytest.mark.parametrize("bands", [False, True])
def test_hist_over_runs_of_several_chunks(gpu, bands):
    """2,051 chunks, two per workgroup, the last workgroup with one ragged chunk; with the band map: waves and whole chunks
    without a measurement, first or later in a workgroup's run, and workgroups that measured nothing."""
    from gs_slam import view_redundancy

    k = (R.band_case if bands else R.case)(*LONG)
    assert R.plan(*LONG[:3])[2] == 2 and R.plan(*LONG[:3])[0] % 256 != 0
    if bands:
        assert all(len(s) for s in R.skip_situations(k["z"], LONG[2]))
    z, table = _tensors(gpu, k)
    seen = R.seen_f32(k["z"], k["cam"], k["views"], LONG[2], k["near"], 2)
    for s in (-1, 3):
        got = view_redundancy(z, k["cam"], table, LONG[3], s, stride=LONG[2], near=k["near"], border=2).cpu().numpy()
        want = RR.hist_from_seen(seen, s)
        assert np.array_equal(got, want), (s, got, want)


def _offset_views(k):
    """The views of an overlap_ref case with assorted principal-point offsets, every third one without."""
    offs = (P.OFFSETS[0], (0.0, 0.0), P.OFFSETS[1], (-3.25, 6.5))
    return [P.offset_camera(v, offs[i % 4]) if offs[i % 4] != (0.0, 0.0) else v for i, v in enumerate(k["views"])]


def test_hist_with_principal_point_offsets(gpu):
    from gaussian import _lib
    from gs_geometry import principal_point_offset
    from gs_seed import seed_camera, seed_camera_pp
    from gs_slam import view_redundancy

    Hc, Wc, stride, n_views = 37, 53, 1, 65
    k = R.case(Hc, Wc, stride, n_views)
    cam, views = P.offset_camera(k["cam"], (7.3, -4.6)), _offset_views(k)
    z, table = _tensors(gpu, k)
    table_pp = torch.tensor([principal_point_offset(v) for v in views], dtype=torch.float32, device=gpu)
    for border, s in ((0, -1), (2, 0), (2, 64)):
        got = view_redundancy(z, cam, table, n_views, s, stride=stride, near=k["near"], border=border, table_pp=table_pp)
        want = RR.hist_f32(k["z"], cam, views, s, stride, k["near"], border)
        assert np.array_equal(got.cpu().numpy(), want), (border, s, got, want)
    centred = RR.hist_f32(k["z"], k["cam"], k["views"], 0, stride, k["near"], 2)
    assert not np.array_equal(RR.hist_f32(k["z"], cam, views, 0, stride, k["near"], 2), centred)  # (the offsets matter)
    # the source's offset alone, no table
    got = view_redundancy(z, cam, table, n_views, 5, stride=stride, near=k["near"], border=0).cpu().numpy()
    assert np.array_equal(got, RR.hist_f32(k["z"], cam, k["views"], 5, stride, k["near"], 0))
    # no offset anywhere: gs_view_redundancy's bits -- through the PP entry point without a table (the call IS
    # gs_view_redundancy) and through the PP kernel on a table of zeros
    plain = view_redundancy(z, k["cam"], table, n_views, 0, stride=stride, near=k["near"], border=2)
    assert np.array_equal(plain.cpu().numpy(), centred)
    zeros = torch.zeros_like(table_pp)
    assert torch.equal(view_redundancy(z, k["cam"], table, n_views, 0, stride, k["near"], 2, table_pp=zeros), plain)
    cpp, opts = seed_camera_pp(k["cam"]), _lib.GsOverlapOpts(stride, k["near"], 2)
    assert (cpp.pp_dx, cpp.pp_dy) == (0.0, 0.0) and bytes(cpp.cam) == bytes(seed_camera(k["cam"]))
    ws = torch.empty(int(_lib.gs_view_redundancy_workspace_bytes(Hc, Wc, stride)), dtype=torch.uint8, device=gpu)
    hist = torch.full((9,), -1, dtype=torch.int64, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(_lib.gs_view_redundancy_pp(z.data_ptr(), C.byref(cpp), table.data_ptr(), None, n_views, 0, C.byref(opts),
                                              hist.data_ptr(), ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream(gpu).cuda_stream), "gs_view_redundancy_pp")
    assert torch.equal(hist, plain)


@pytest.mark.parametrize("Hc,Wc,stride", [(120, 160, 2)])
def test_hist_against_the_overlap_kernel(gpu, Hc, Wc, stride):
    """Three views, none of whose points can reach bin 7: sum(b hist[b]) is the sum of gs_view_overlap's counts without row
    self_index, the point counts agree, and with no row left out bin 0 is gs_view_overlap's "seen by nobody"."""
    from gs_slam import view_overlap, view_redundancy

    k = R.case(Hc, Wc, stride, 3)
    z, table = _tensors(gpu, k)
    counts = view_overlap(z, k["cam"], table, 3, stride=stride, near=k["near"], border=2).cpu().numpy()
    for s in (-1, 0, 1, 2):
        h = view_redundancy(z, k["cam"], table, 3, s, stride=stride, near=k["near"], border=2).cpu().numpy()
        others = np.delete(counts[:3], s) if s >= 0 else counts[:3]
        assert h[7] == 0 and (np.arange(8) * h[:8]).sum() == others.sum() > 0 and h[8] == counts[3]
        if s < 0:
            assert h[0] == counts[4]


@pytest.mark.parametrize("Hc,Wc,stride,n_views", [(37, 53, 1, 65), (120, 160, 2, 256)])
def test_result_is_a_pure_function_of_the_inputs(gpu, Hc, Wc, stride, n_views):
    """The same call into a workspace and a hist_dev filled with 0xFF bytes gives the same nine numbers; `out` and `ws` of
    the caller's are written and used."""
    from gaussian import _lib
    from gs_seed import seed_camera
    from gs_slam import view_redundancy

    k = R.case(Hc, Wc, stride, n_views)
    z, table = _tensors(gpu, k)
    first = view_redundancy(z, k["cam"], table, n_views, 64, stride=stride, near=k["near"], border=2)
    cam, opts = seed_camera(k["cam"]), _lib.GsOverlapOpts(stride, k["near"], 2)
    nbytes = int(_lib.gs_view_redundancy_workspace_bytes(Hc, Wc, stride))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
    hist = torch.full((9,), -1, dtype=torch.int64, device=gpu)  # (0xFF in every byte)
    _lib.check(_lib.gs_view_redundancy(z.data_ptr(), C.byref(cam), table.data_ptr(), n_views, 64, C.byref(opts),
                                       hist.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
               "gs_view_redundancy")
    assert torch.equal(first, hist)
    assert np.array_equal(first.cpu().numpy(), RR.hist_f32(k["z"], k["cam"], k["views"], 64, stride, k["near"], 2))
    many = torch.full((3, 9), -1, dtype=torch.int64, device=gpu)
    ws.fill_(0xFF)
    assert view_redundancy(z, k["cam"], table, n_views, 64, stride, k["near"], 2, out=many[1], ws=ws).data_ptr() == many[1].data_ptr()
    assert torch.equal(many[1], first) and bool((many[0] == -1).all()) and bool((many[2] == -1).all())
    with pytest.raises(ValueError, match="out"):
        view_redundancy(z, k["cam"], table, n_views, 64, stride, k["near"], 2, out=many[:, 0])
    with pytest.raises(RuntimeError, match="self_index"):
        view_redundancy(z, k["cam"], table, n_views, n_views, stride, k["near"], 2)


# --------------------------------------------------------------------------------------------------------- KeyframeSet
def test_keyframe_set_removes_a_view(gpu):
    """Five views, remove(2): table / table_pp rows equal those of a set built from the remaining four in order, the freed row
    is zero, ids keep their values and the next add gets a new one; a full set accepts an add after a remove; redundancy()
    equals the restatement per row, and the overlap counts afterwards are those of the remaining views."""
    from gs_slam import KeyframeSet, view_overlap

    Hc, Wc, stride = 37, 53, 1
    k = R.case(Hc, Wc, stride, 65)
    views = [P.offset_camera(v, (2.5, -1.25)) if i == 3 else v for i, v in enumerate(k["views"][:6])]
    # each keyframe's own range map, of its own size (view 2 is larger): the shared surface with another seed's holes
    zs = [R.range_map(v.height, v.width, seed=90 + i) for i, v in enumerate(views)]
    assert zs[2].shape == (Hc + 6, Wc + 11) and zs[5].shape == (Hc, Wc)
    zt = [torch.from_numpy(z).to(gpu) for z in zs]
    img = torch.zeros((Hc, Wc, 3), device=gpu)
    ks = KeyframeSet(capacity=5, device=gpu)
    for i in range(5):
        assert ks.add(views[i], img, zt[i]) == i
    assert ks.ids == [0, 1, 2, 3, 4] and ks.n_added == 5
    with pytest.raises(RuntimeError, match="full"):
        ks.add(views[5], img, zt[5])
    for bad in (5, -1, 17):
        with pytest.raises(IndexError):
            ks.remove(bad)

    def check_redundancy(kset, order):
        got = kset.redundancy(stride=stride, near=k["near"], border=2)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (len(order), 9)
        cams = [views[i] for i in order]
        for row, i in enumerate(order):
            want = RR.hist_f32(zs[i], views[i], cams, row, stride, k["near"], 2)
            assert np.array_equal(got[row], want), (order, row, got[row], want)

    check_redundancy(ks, [0, 1, 2, 3, 4])
    ks.remove(2)
    rest = [0, 1, 3, 4]
    fresh = KeyframeSet(capacity=5, device=gpu)
    for i in rest:
        fresh.add(views[i], img, zt[i])
    assert len(ks) == 4 and ks.ids == [0, 1, 3, 4] and fresh.ids == [0, 1, 2, 3]
    assert torch.equal(ks.table, fresh.table) and torch.equal(ks.table_pp, fresh.table_pp)
    assert not ks.table[4].any() and not ks.table_pp[4].any() and ks.table[3].any() and ks.table_pp[2].any()
    assert ks._offsets == fresh._offsets and ks._min_size == fresh._min_size
    assert all(a is b for a, b in zip(ks.ranges, [zt[i] for i in rest])) and len(ks.cameras) == len(ks.images) == 4
    check_redundancy(ks, rest)
    want = P.overlap_counts_f32(zs[5], k["cam"], [views[i] for i in rest], stride, k["near"], 2)
    assert np.array_equal(ks.overlap(zt[5], k["cam"], stride=stride, near=k["near"], border=2), want)
    got = view_overlap(zt[5], k["cam"], ks.table, 4, stride, k["near"], 2, ks.table_pp).cpu().numpy()
    assert np.array_equal(got, want)
    assert ks.add(views[5], img, zt[5]) == 4 and ks.ids == [0, 1, 3, 4, 5] and ks.n_added == 6
    check_redundancy(ks, rest + [5])
    ks.remove(4)  # the last position: nothing moves, the row is zeroed
    assert ks.ids == [0, 1, 3, 4] and torch.equal(ks.table, fresh.table)
    ks.remove(0)
    assert ks.ids == [1, 3, 4] and torch.equal(ks.table[:3], fresh.table[1:4]) and not ks.table[3:].any()
    # a set at capacity 3 accepts an add after a remove; the offset view gone, the plain kernel's path again
    small = KeyframeSet(capacity=3, device=gpu)
    for i in (0, 1, 2):
        small.add(views[i], img, zt[i])
    with pytest.raises(RuntimeError, match="full"):
        small.add(views[4], img, zt[4])
    small.remove(1)
    assert small.add(views[4], img, zt[4]) == 2 and small.ids == [0, 2, 3] and len(small) == 3
    check_redundancy(small, [0, 2, 4])
    want = R.counts_f32(zs[5], k["cam"], [views[i] for i in (0, 2, 4)], stride, k["near"], 0)
    assert np.array_equal(small.overlap(zt[5], k["cam"], stride=stride, near=k["near"], border=0), want)
    one = KeyframeSet(capacity=2, device=gpu)
    one.add(views[0], img, zt[0])
    h = one.redundancy(stride=stride, near=k["near"])
    assert h.shape == (1, 9) and h[0, 0] == h[0, 8] > 0
    one.remove(0)
    assert len(one) == 0 and one._min_size is None and not one.table.any()
    with pytest.raises(RuntimeError, match="empty"):
        one.redundancy()
