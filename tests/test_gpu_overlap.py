"""GPU tier of the covisibility count (csrc/overlap.hip through gs_slam.view_overlap / KeyframeSet): every count against the
float32 restatement of tests/overlap_ref.py exactly and inside the float64 band, bitwise repeatable whatever the workspace
held, the same on a side stream, and the keyframe table grown row by row against a fresh one."""
import ctypes as C

import numpy as np
import pytest
import torch

import overlap_ref as R

pytestmark = pytest.mark.gpu


def _tensors(gpu, k):
    return torch.from_numpy(k["z"]).to(gpu), torch.from_numpy(R.table_rows(k["views"])).to(gpu)


@pytest.mark.parametrize("Hc,Wc,stride,n_views", R.cases())
def test_counts_equal_the_float32_restatement(gpu, Hc, Wc, stride, n_views):
    """All n_views + 2 entries, no point left out, for border 0 and 4; inside the float64 band; the closed-form views."""
    from gs_slam import view_overlap

    k = R.case(Hc, Wc, stride, n_views)
    z, table = _tensors(gpu, k)
    for border in (0, 4):
        got = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=border).cpu().numpy()
        want = R.counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], border)
        assert got.dtype == np.int64 and got.shape == (n_views + 2,)
        assert np.array_equal(got, want), (border, np.nonzero(got != want)[0][:8], got[:8], want[:8])
        c64, und = R.counts_f64(k["z"], k["cam"], k["views"], stride, k["near"], border)
        assert (np.abs(got[:n_views] - c64[:n_views]) <= und.sum(1)).all() and got[n_views] == c64[n_views]
        assert abs(int(got[n_views + 1]) - int(c64[n_views + 1])) <= int(und.any(0).sum())
        assert got[0] == R.own_view_count(k["z"], stride, border)
        if n_views > 1:
            assert got[1] == 0


@pytest.mark.parametrize("Hc,Wc,stride,n_views", [(37, 53, 1, 65), (120, 160, 2, 256)])
def test_result_is_a_pure_function_of_the_inputs(gpu, Hc, Wc, stride, n_views):
    """Two runs bitwise equal, one of them on a workspace and a counts_dev pre-filled with 0xFF; a call on a side stream
    gives the same counts."""
    from gaussian import _lib
    from gs_seed import seed_camera
    from gs_slam import view_overlap

    k = R.case(Hc, Wc, stride, n_views)
    z, table = _tensors(gpu, k)
    first = view_overlap(z, k["cam"], table, n_views, stride=stride, near=k["near"], border=4)
    cam, opts = seed_camera(k["cam"]), _lib.GsOverlapOpts(stride, k["near"], 4)
    nbytes = int(_lib.gs_view_overlap_workspace_bytes(Hc, Wc, stride, n_views))

    def raw(stream):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
        counts = torch.full((n_views + 2,), -1, dtype=torch.int64, device=gpu)  # (0xFF in every byte)
        _lib.check(_lib.gs_view_overlap(z.data_ptr(), C.byref(cam), table.data_ptr(), n_views, C.byref(opts),
                                        counts.data_ptr(), ws.data_ptr(), nbytes, stream.cuda_stream), "gs_view_overlap")
        return counts

    second = raw(torch.cuda.current_stream())
    assert torch.equal(first, second)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        third = raw(side)
    side.synchronize()
    assert torch.equal(first, third)
    assert np.array_equal(first.cpu().numpy(), R.counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], 4))


def test_keyframe_set_grows_row_by_row(gpu):
    """Counts after `add` of view k equal a fresh table's of k + 1 rows; `overlap` equals `view_overlap`; a full set
    refuses another view, and so do an empty one and a border that leaves nothing."""
    from gs_slam import KeyframeSet, view_overlap

    Hc, Wc, stride = 37, 53, 1
    k = R.case(Hc, Wc, stride, 65)
    z, table = _tensors(gpu, k)
    n = 7
    ks = KeyframeSet(capacity=n, device=gpu)
    with pytest.raises(RuntimeError, match="empty"):
        ks.overlap(z, k["cam"])
    img = torch.zeros((Hc, Wc, 3), device=gpu)
    for i in range(n):
        assert ks.add(k["views"][i], img, z) == i and len(ks) == i + 1
        got = ks.overlap(z, k["cam"], stride=stride, near=k["near"], border=2)
        fresh = view_overlap(z, k["cam"], table[: i + 1].contiguous(), i + 1, stride=stride, near=k["near"], border=2)
        assert isinstance(got, np.ndarray) and np.array_equal(got, fresh.cpu().numpy())
        assert np.array_equal(got, R.counts_f32(k["z"], k["cam"], k["views"][: i + 1], stride, k["near"], 2))
    assert torch.equal(ks.table, table[:n])
    with pytest.raises(RuntimeError, match="full"):
        ks.add(k["views"][n], img, z)
    assert len(ks) == n
    with pytest.raises(RuntimeError, match="border"):
        ks.overlap(z, k["cam"], border=19)  # 2 x 19 >= 37
