"""CPU tier of the forward issued in ranges of project slices (gs_frame_forward_project + gs_frame_forward_rest, include/
gs_abi.h): the plan `gs_frame_project_slices` states -- how many slices of the Gaussian array a frame's project stage is
made of, and how many Gaussians each holds -- against the restatement of it in Python that the view-parallel trainer cuts
its exchange slices with (gs_dp.project_slice_size, FlatGaussianParams.slice_bounds).  If the two drifted apart, a range of
exchange slices would name other Gaussians than the project slices issued for it.

Descriptors carry fake device addresses (tests/gs_testutil.fake_frame): gs_frame_project_slices validates, answers on the
host and enqueues nothing.  The constants below are restated beside the source line they come from: whoever moves one
moves the test."""
import ctypes as C

import pytest
import torch

import gs_dp
from gs_testutil import fake_frame

# csrc/gs_frame_layout.h: `#define GS_BIN_SLICES 256` -- the most slices a project stage is cut into ...
GS_BIN_SLICES = 256
# ... gs_strip_plan_for: `per = gs_div_up(gs_div_up(n, GS_BIN_SLICES), 256) * 256` -- in whole blocks of 256 Gaussians
PROJECT_BLOCK = 256
# csrc/gs_frame_layout.h: `#define GS_STRIP_AUTO_MIN_N 131072` -- from here on a sort_mode-2 frame takes the strip variant
# by itself
GS_STRIP_AUTO_MIN_N = 131072
# csrc/gs_frame_layout.h: `#define GS_BIN_MAX_TILES 32768` -- ... and so does a frame of more tiles than this, whatever its N
GS_BIN_MAX_TILES = 32768
# csrc/gs_common.h: `#define GS_TILE 16`
GS_TILE = 16
# csrc/gs_frame_layout.h: `#define GS_STRIP_W 8`, `#define GS_STRIP_MAX 8192`, `#define GS_STRIP_ID_BITS 26` -- the limits of
# the strip variant (gs_strip_plan_for: `p.ok = N < (1ll << GS_STRIP_ID_BITS) && p.geom.NS <= GS_STRIP_MAX`)
GS_STRIP_W, GS_STRIP_MAX, GS_STRIP_ID_BITS = 8, 8192, 26

COUNTS = [1, 255, 256, 257, 65_536, 65_537, 131_071, 131_072, 376_467, 2_400_000, (1 << 26) - 1]
SIZES = [(128, 96), (333, 201), (1920, 1080), (3840, 2160)]


def _plan(f):
    from gaussian import _lib

    slices, per = C.c_int32(-1), C.c_int64(-1)
    rc = _lib.gs_frame_project_slices(C.byref(f), C.byref(slices), C.byref(per))
    assert rc == 0, (rc, _lib.gs_last_error())
    return slices.value, per.value


def _frame(n, w, h, flags=0, sort_mode=2):
    f = fake_frame(N=n, W=w, H=h)
    f.flags |= flags
    f.sort_mode = sort_mode
    return f


def _tiles(w, h):
    return -(-w // GS_TILE), -(-h // GS_TILE)


def _takes_strips_by_itself(n, w, h):
    """gs_frame_uses_strips without a forcing flag: `f->N >= GS_STRIP_AUTO_MIN_N || ntx * nty > GS_BIN_MAX_TILES`."""
    ntx, nty = _tiles(w, h)
    return n >= GS_STRIP_AUTO_MIN_N or ntx * nty > GS_BIN_MAX_TILES


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("n", COUNTS)
def test_plan_of_a_strip_frame_is_the_one_python_restates(n, w, h):
    from gaussian import _lib

    ntx, nty = _tiles(w, h)
    assert n < (1 << GS_STRIP_ID_BITS) and -(-ntx // GS_STRIP_W) * nty <= GS_STRIP_MAX  # inside the strip variant's limits
    want_per = gs_dp.project_slice_size(n)
    frames = [("GS_FRAME_STRIP_BIN", _frame(n, w, h, _lib.GS_FRAME_STRIP_BIN))]
    if _takes_strips_by_itself(n, w, h):
        frames.append(("no flag", _frame(n, w, h)))
    for what, f in frames:
        slices, per = _plan(f)
        assert per == want_per, (what, n, per, want_per)
        assert slices == -(-n // per) and 1 <= slices <= GS_BIN_SLICES, (what, n, slices, per)
        assert per % PROJECT_BLOCK == 0, (what, n, per)
        assert (slices - 1) * per < n <= slices * per  # the last slice holds at least one Gaussian
    # a frame of this size without a forcing flag: ranges exactly where the library takes the strip variant by itself
    slices, per = _plan(_frame(n, w, h))
    assert (slices > 0) == _takes_strips_by_itself(n, w, h), (n, w, h, slices)
    assert (per > 0) == (slices > 0)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("n", COUNTS)
def test_frames_that_cannot_be_issued_in_ranges_say_zero(n, w, h):
    from gaussian import _lib

    # the other binning variants of sort_mode 2, asked for by flag (also together with GS_FRAME_STRIP_BIN: gs_frame_uses_strips
    # looks at them first) ...
    for flags in (_lib.GS_FRAME_TABLE_BIN, _lib.GS_FRAME_SLICE_SORT, _lib.GS_FRAME_TABLE_BIN | _lib.GS_FRAME_STRIP_BIN,
                  _lib.GS_FRAME_SLICE_SORT | _lib.GS_FRAME_STRIP_BIN):
        assert _plan(_frame(n, w, h, flags)) == (0, 0), (n, flags)
    # ... the radix paths, whatever the flags ...
    for mode in (0, 1):
        assert _plan(_frame(n, w, h, 0, sort_mode=mode)) == (0, 0), (n, mode)
        assert _plan(_frame(n, w, h, _lib.GS_FRAME_STRIP_BIN, sort_mode=mode)) == (0, 0), (n, mode)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_empty_and_small_unforced_frames_say_zero(w, h):
    from gaussian import _lib

    assert _plan(_frame(0, w, h)) == (0, 0)
    assert _plan(_frame(0, w, h, _lib.GS_FRAME_STRIP_BIN)) == (0, 0)
    for n in (1, 3_001, GS_STRIP_AUTO_MIN_N - 1):
        assert not _takes_strips_by_itself(n, w, h)
        assert _plan(_frame(n, w, h)) == (0, 0), n
    assert _plan(_frame(GS_STRIP_AUTO_MIN_N, w, h))[0] == GS_BIN_SLICES  # 131,072 = 256 slices of 512


def test_null_outputs_are_refused():
    from gaussian import _lib

    f = _frame(1000, 128, 96, _lib.GS_FRAME_STRIP_BIN)
    per = C.c_int64()
    assert _lib.gs_frame_project_slices(C.byref(f), None, C.byref(per)) == -1  # GS_E_INVALID
    assert b"null pointer" in _lib.gs_last_error()


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", COUNTS)
def test_exchange_slices_are_whole_project_slices(n, k):
    """FlatGaussianParams cuts the Gaussian array into exchange slices whose bounds the trainer divides by the project slice
    size to name project slices (gs_train.Trainer._project_ahead): every bound but the array's padded end must be a whole
    multiple of the per_slice the LIBRARY states for a frame of these Gaussians.  (Tensors on the meta device: the constructor
    runs as it is, nothing of the 2^26-Gaussian case is allocated.)"""
    from gaussian import _lib

    slices, per = _plan(_frame(n, 128, 96, _lib.GS_FRAME_STRIP_BIN))
    params = [torch.empty(n, c, device="meta") for c in (3, 4, 3)] + [torch.empty(n, device="meta"),
                                                                       torch.empty(n, 3, device="meta")]
    flat = gs_dp.FlatGaussianParams(params, n_slices=k)
    assert flat.project_slice == per
    b = flat.slice_bounds
    assert b[0] == 0 and b[-1] == flat.n_pad >= n and b == sorted(set(b)) and 1 <= flat.n_slices <= k, b
    assert all(x % per == 0 for x in b[:-1]), (n, k, per, b)
    # the project slices the trainer derives for exchange slice j -- [g0 // per, ceil(g1 / per)) -- tile [0, slices) exactly
    cover = []
    for j in range(flat.n_slices):
        g0, g1 = flat.slice_gaussians(j)
        cover.append((g0 // per, -(-g1 // per)))
    assert cover[0][0] == 0 and cover[-1][1] == slices, (cover, slices)
    assert all(a[1] == c[0] for a, c in zip(cover, cover[1:])), cover
