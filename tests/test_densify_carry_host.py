"""CPU tier of the carried densification (include/gs_abi.h: gs_densify_apply_state): the symbol and its ctypes binding, every
refusal on fake pointers (each comes before anything is enqueued), N = 0, the unchanged workspace query, the Python surface, and
the numpy restatement (tests/densify_carry_ref.py) against hand-written cases.  No kernel is launched."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
N = 1000


def _arrays(n=10, widths=(3, 4, 3, 1, 3), **kw):
    from gaussian import _lib

    a = _lib.GsPruneArrays()
    a.n = n
    for k in range(max(min(n, 16), 0)):
        a.width[k] = widths[k % len(widths)]
        a.src[k] = FAKE + k * (1 << 28)
        a.dst[k] = FAKE + (k + 32) * (1 << 28)
    for k, v in kw.items():
        field, index = k.split("_")
        getattr(a, field)[int(index)] = v
    return a


def test_symbol_is_exported_and_bound():
    from gaussian import _lib

    assert "gs_densify_apply_state" in _lib.EXPORTS
    assert getattr(_lib.lib, "gs_densify_apply_state") is not None and callable(_lib.gs_densify_apply_state)
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    assert "int gs_densify_apply_state(const gs_prune_arrays *arrays, int64_t N, int64_t capacity," in header
    assert header.index("} gs_prune_arrays;") < header.index("int gs_densify_apply_state(")  # declared behind its argument
    assert "purely additive (clients built against the earlier version 8 header are unaffected): gs_densify_apply_state" \
        in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    # the ctypes mirror: the struct of gs_prune_apply as it stands, then N, capacity, counts, workspace, bytes, stream
    f = _lib.gs_densify_apply_state
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(_lib.GsPruneArrays), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p]
    assert C.sizeof(_lib.GsPruneArrays) == 72 + 2 * 16 * 8 and _lib.GS_PRUNE_MAX_ARRAYS == 16


def test_densify_workspace_query_is_unchanged():
    """cls (4 bytes per row) and three counts per 256 rows, each part rounded up to 256 bytes: what gs_densify_classify always
    asked for -- the new call reads that workspace and needs nothing more."""
    from gaussian import _lib

    def want(n):
        rows = max(n, 1)
        blocks = -(-rows // 256)
        return -(-4 * rows // 256) * 256 + -(-12 * blocks // 256) * 256

    for n in (0, 1, 255, 256, 257, 1000, 262_145, 376_000, 2_400_000, (1 << 31) - 1):
        assert _lib.gs_densify_workspace_bytes(n) == want(n), n
    assert _lib.gs_densify_workspace_bytes(-1) == 0


def test_apply_state_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_densify_workspace_bytes(N)
    CNT, WS = FAKE + (1 << 24), FAKE + (2 << 24)

    def call(arrays="default", n=N, capacity=2 * N, cnt=CNT, ws=WS, nbytes=ws_bytes):
        a = _arrays() if arrays == "default" else arrays
        return _lib.gs_densify_apply_state(C.byref(a) if a is not None else None, n, capacity, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert msg.startswith(b"gs_densify_apply_state: invalid argument: ") and word in msg, (kw, msg)

    refused(b"arrays is null", arrays=None)
    refused(b"counts_dev is null", cnt=None)
    for k in range(10):
        refused(b"a src or dst pointer is null", arrays=_arrays(**{f"src_{k}": None}))
        refused(b"a src or dst pointer is null", arrays=_arrays(**{f"dst_{k}": None}))
    refused(b"a src or dst pointer is null", arrays=_arrays(n=16, src_15=None))
    for n_arrays in (0, -1, 17, 1 << 20):
        refused(b"the number of arrays must lie in 1 .. 16", arrays=_arrays(n=n_arrays))
    for w in (0, -1, -48):
        refused(b"a row width must be >= 1", arrays=_arrays(width_2=w))
    for n in (-1, 1 << 31):
        refused(b"N out of range", n=n, nbytes=1 << 40)
    refused(b"capacity must not be negative", capacity=-1)
    a = _arrays()
    refused(b"a dst array is a src array", arrays=_arrays(dst_3=a.src[3]))   # in place
    refused(b"a dst array is a src array", arrays=_arrays(dst_0=a.src[9]))   # ... or onto another source
    refused(b"workspace null, misaligned or too small", ws=None)
    refused(b"workspace null, misaligned or too small", nbytes=ws_bytes - 1)
    refused(b"workspace null, misaligned or too small", nbytes=0)
    refused(b"workspace null, misaligned or too small", ws=WS + 2)
    # N = 0 is valid and moves nothing; so is a destination of no rows (the caller saw total = 0)
    assert call(n=0) == 0 and call(capacity=0) == 0
    # an array of no rows has no address
    assert call(arrays=_arrays(src_1=None), n=0) == 0 and call(arrays=_arrays(dst_1=None), capacity=0) == 0


def test_python_surface():
    import torch

    import gs_densify
    import gs_train

    sig = inspect.signature(gs_densify.densify_apply_state)
    assert list(sig.parameters) == ["src", "dst", "n", "counts", "ws", "capacity"]
    assert list(inspect.signature(gs_densify.densify_classify).parameters)[:4] == ["params", "grad", "taus", "delete_thresh"]
    assert callable(gs_densify.densify_apply)
    # adaptive_control keeps the signature it had
    assert list(inspect.signature(gs_densify.adaptive_control).parameters) == [
        "params", "grad", "taus", "delete_thresh", "scale_activation", "grad_thresh", "grad_aggregation", "use_clone",
        "use_split", "clone_dt", "generator", "draws"]
    with pytest.raises(RuntimeError):  # a HIP kernel: no CPU fallback
        gs_densify.densify_apply_state([torch.zeros(4, 3)], [torch.zeros(4, 3)], 4, torch.zeros(4, dtype=torch.int64),
                                       torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="1 .. 16"):
        gs_densify.densify_apply_state([], [], 0, torch.zeros(4, dtype=torch.int64), torch.zeros(1024, dtype=torch.uint8))
    assert inspect.signature(gs_train.Trainer.__init__).parameters["densify_carry"].default is False
    sig = inspect.signature(gs_train.Trainer.adaptive_control)
    assert list(sig.parameters) == ["self", "i_iter", "densify", "carry_state"]
    assert sig.parameters["densify"].default is True and sig.parameters["carry_state"].default is None


def test_state_kernel_is_small_and_free_of_scratch():
    """A streaming kernel: 64 VGPRs and fewer keep eight waves per SIMD, and the array table, indexed with a loop counter, must
    not be copied to scratch (it would be paid per array per workgroup).  LDS: the 256-entry slot -> row table and
    block_scan3's 3 x 4 wave totals, nothing else."""
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    kernels = {}
    for elf in code_objects(open(LIB, "rb").read()):
        kernels.update(kernel_metadata(elf))
    hits = [k for k in kernels if "densify_apply_state_kernel" in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    assert k[".group_segment_fixed_size"] == 1024 + 48


def _case(cls, width=2):
    from densify_carry_ref import apply_state, counts

    cls = np.asarray(cls, np.int32)
    n = len(cls)
    a = (np.arange(n * width, dtype=np.float32) + 1).reshape(n, width)  # row i = (2 i + 1, 2 i + 2): no zero anywhere
    b = -(np.arange(n, dtype=np.float32) + 1)
    return counts(cls), apply_state(cls, [a, b]), a, b


def test_restatement_on_hand_written_cases():
    (k, c, s), (da, db), a, b = _case([1, 1, 1, 1])  # all kept: a copy
    assert (k, c, s) == (4, 0, 0) and np.array_equal(da, a) and np.array_equal(db, b)
    (k, c, s), (da, db), a, b = _case([0, 0, 0])  # all deleted: nothing
    assert (k, c, s) == (0, 0, 0) and da.shape == (0, 2) and db.shape == (0,)
    (k, c, s), (da, db), a, b = _case([3, 3, 3])  # all split: three zero slots and three zero second samples
    assert (k, c, s) == (3, 0, 3) and da.shape == (6, 2) and not da.any() and db.shape == (6,) and not db.any()
    (k, c, s), (da, db), a, b = _case([2, 2])  # all cloned: the rows themselves, then two zero clones
    assert (k, c, s) == (2, 2, 0) and np.array_equal(da[:2], a) and not da[2:].any() and da.shape == (4, 2)
    assert np.array_equal(db, [-1, -2, 0, 0])
    (k, c, s), (da, db), a, b = _case([3, 0, 2, 1, 0])  # one of each (and a second deleted row at the end)
    assert (k, c, s) == (3, 1, 1)
    assert da.tolist() == [[0, 0], [5, 6], [7, 8], [0, 0], [0, 0]]  # split slot, clone's own row, kept row, clone, 2nd sample
    assert db.tolist() == [0, -3, -4, 0, 0]
    for d in (da, db):  # zeros are +0
        assert not np.signbit(d[d == 0]).any() and d.dtype == np.float32


def test_restatement_classes_follow_the_oracle():
    """The classes against oracle/densify_ref.py's own counts on a set where every class occurs, and a hand-made row of each
    class; switching clone or split off turns those rows into kept ones."""
    from densify_carry_ref import classes, counts
    from oracle import densify_ref

    g = np.random.default_rng(3)
    n = 500
    pos, quat = g.normal(size=(n, 3)).astype(np.float32), g.normal(size=(n, 4)).astype(np.float32)
    scale = (g.uniform(0.005, 0.12, size=(n, 3)) * g.choice([-1, 1], size=(n, 3))).astype(np.float32)
    opa, rgb = g.normal(-2.0, 2.5, size=n).astype(np.float32), g.normal(size=(n, 3)).astype(np.float32)
    grad = (g.normal(size=(n, 3)) * 3e-4).astype(np.float32)
    eps = g.normal(size=(n, 3)).astype(np.float32)
    for use_clone, use_split in ((True, True), (False, True), (True, False), (False, False)):
        cls = classes(scale, opa, grad, "abs", "max", use_clone, use_split)
        want = densify_ref.adaptive_control(pos, quat, scale, opa, rgb, grad, 0.05, 0.17, eps, eps, use_clone=use_clone,
                                            use_split=use_split)[5]
        assert counts(cls) == want
        if use_clone and use_split:
            assert min(want) > 0 and (cls == 0).any() and (cls == 1).any()
    s = np.array([[0.01, 0.01, 0.01], [0.01, 0.01, 0.01], [0.04, 0.04, 0.04], [0.2, 0.2, 0.2], [0.01, 0.01, 0.01]], np.float32)
    o = np.array([0.0, 0.0, 0.0, 0.0, -9.0], np.float32)
    gr = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [1, 1, 1], [1, 1, 1]], np.float32)
    assert classes(s, o, gr).tolist() == [1, 2, 3, 0, 0]
    assert classes(s, o, gr, use_clone=False, use_split=False).tolist() == [1, 1, 1, 0, 0]
    assert classes(s, o, gr, taus=0.1, delete_thresh=1.0, grad_thresh=2.0).tolist() == [1, 1, 1, 1, 0]
