"""CPU tier of the map edit (include/gs_abi.h: gs_prune_workspace_bytes, gs_prune_classify, gs_prune_apply): the symbols and
their ctypes bindings, the workspace size query, every refusal on fake pointers (each comes before anything is enqueued), the
Python surface and its defaults, the float32 restatement's decision, and the register / scratch budgets of the new kernels
read from the built code objects.  No kernel is launched."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
N = 1000


def _opts(**kw):
    from gaussian import _lib

    o = _lib.GsPruneOpts(-5.0, math.inf, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _arrays(n=5, widths=(3, 4, 3, 1, 3), **kw):
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


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_prune_workspace_bytes", "gs_prune_classify", "gs_prune_apply"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_prune_workspace_bytes(", "int gs_prune_classify(", "int gs_prune_apply(", "} gs_prune_opts;",
                 "} gs_prune_arrays;", "#define GS_PRUNE_MAX_ARRAYS 16"):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    assert _lib.GS_PRUNE_MAX_ARRAYS == 16
    # the header's layouts: three 4-byte fields; n + 16 widths (68 bytes, padded to 72) + 2 x 16 pointers
    assert C.sizeof(_lib.GsPruneOpts) == 12 and C.sizeof(_lib.GsPruneArrays) == 72 + 2 * 16 * 8
    assert _lib.GsPruneArrays.src.offset == 72 and _lib.GsPruneArrays.dst.offset == 72 + 128


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_prune_workspace_bytes
    sizes = [0, 1, 255, 256, 257, 4099, 262_144 + 257, 376_000, 2_400_000, (1 << 31) - 1]
    got = [q(n) for n in sizes]
    for b in got:
        assert b > 0 and b % 256 == 0
    assert got == sorted(got) and got[-1] > got[0]  # monotone
    # a 64-bit ballot per 64 rows and a 32-bit count per 256: an eighth of a byte and a sixty-fourth per row
    assert 2_400_000 * (1 / 8 + 1 / 64) <= got[8] <= 2_400_000 * (1 / 8 + 1 / 64) + 1024
    for bad in (-1, -256, -(1 << 40)):
        assert q(bad) == 0


def test_classify_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_prune_workspace_bytes(N)
    SCALE, OPA, CNT, WS = (FAKE + i * (1 << 24) for i in range(4))

    def call(scale=SCALE, opa=OPA, n=N, opts="default", cnt=CNT, ws=WS, nbytes=ws_bytes):
        o = _opts() if opts == "default" else opts
        return _lib.gs_prune_classify(scale, opa, n, C.byref(o) if o is not None else None, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_prune_classify" in msg and word in msg, (kw, msg)

    refused(b"null", scale=None)
    refused(b"null", opa=None)
    refused(b"null", cnt=None)
    refused(b"null", opts=None)
    for n in (-1, -1000, 1 << 31):
        refused(b"N out of range", n=n, nbytes=1 << 40)
    for v in (math.inf, -math.inf, math.nan):
        refused(b"opa_logit_min", opts=_opts(opa_logit_min=v))
    refused(b"scale_max", opts=_opts(scale_max=math.nan))
    for act in (-1, 2, 7):
        refused(b"scale_activation", opts=_opts(scale_activation=act))
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"workspace", ws=WS + 4)  # misaligned


def test_apply_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_prune_workspace_bytes(N)
    CNT, WS = FAKE + (1 << 24), FAKE + (2 << 24)

    def call(arrays="default", n=N, offset=0, capacity=N, cnt=CNT, ws=WS, nbytes=ws_bytes):
        a = _arrays() if arrays == "default" else arrays
        return _lib.gs_prune_apply(C.byref(a) if a is not None else None, n, offset, capacity, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_prune_apply" in msg and word in msg, (kw, msg)

    refused(b"null", arrays=None)
    refused(b"null", cnt=None)
    for k in range(5):
        refused(b"null", arrays=_arrays(**{f"src_{k}": None}))
        refused(b"null", arrays=_arrays(**{f"dst_{k}": None}))
    refused(b"null", arrays=_arrays(n=16, src_15=None))
    for n_arrays in (0, -1, 17, 1 << 20):
        refused(b"number of arrays", arrays=_arrays(n=n_arrays))
    for w in (0, -1, -48):
        refused(b"width", arrays=_arrays(width_2=w))
    for n in (-1, 1 << 31):
        refused(b"N out of range", n=n, nbytes=1 << 40)
    refused(b"negative", offset=-1)
    refused(b"negative", capacity=-1)
    a = _arrays()
    refused(b"dst array is a src array", arrays=_arrays(dst_3=a.src[3]))   # in place
    refused(b"dst array is a src array", arrays=_arrays(dst_0=a.src[4]))   # ... or onto another source
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", ws=WS + 4)
    # nothing to move: no rows, or arrays that are already full -- nothing to launch, nothing to complain about
    assert call(n=0) == 0 and call(offset=N, capacity=N) == 0 and call(offset=5, capacity=0) == 0
    # an array of no rows has no address
    assert call(arrays=_arrays(src_1=None), n=0) == 0 and call(arrays=_arrays(dst_1=None), capacity=0) == 0


def test_python_surface_and_defaults():
    import torch

    import gs_prune
    import gs_slam
    import gs_train

    sig = inspect.signature(gs_prune.prune_rows)
    assert list(sig.parameters)[:3] == ["scale", "opa", "arrays"]
    for name in ("opa_min", "scale_max", "scale_activation"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert set(gs_prune.DEFAULTS) == {"opa_min", "scale_max"} and 0.0 < gs_prune.DEFAULTS["opa_min"] < 0.02
    assert gs_prune.DEFAULTS["scale_max"] == math.inf
    o = gs_prune.prune_options()
    assert o.scale_activation == 0 and o.scale_max == math.inf
    assert o.opa_logit_min == np.float32(-math.log(1.0 / gs_prune.DEFAULTS["opa_min"] - 1.0))  # converted in double, once
    assert gs_prune.prune_options(0.5, None, "exp").scale_activation == 1
    assert gs_prune.prune_options(0.5, None).opa_logit_min == 0.0
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError):
            gs_prune.prune_options(bad)
    with pytest.raises(RuntimeError):  # a HIP kernel: no CPU fallback
        gs_prune.prune_rows(torch.zeros(4, 3), torch.zeros(4), [torch.zeros(4, 3)], opa_min=0.1)
    sig = inspect.signature(gs_train.Trainer.prune)
    assert list(sig.parameters)[:2] == ["self", "i_iter"]
    for name in ("opa_min", "scale_max", "carry_state"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig.parameters["carry_state"].default is True and sig.parameters["scale_max"].default == math.inf
    assert inspect.signature(gs_train.Trainer.seed_from_view).parameters["carry_state"].default is False
    assert list(inspect.signature(gs_train.Trainer._bind).parameters) == ["self", "params", "i_iter", "carry"]
    assert inspect.signature(gs_train.Trainer._bind).parameters["carry"].default is None
    so = gs_slam.SlamOptions()
    assert so.carry_optimizer is False and so.prune_every == 0 and so.prune_opa_min == 0.005 and so.prune_scale_max is None
    assert gs_slam.SlamFrame(rot=None, tran=None, tracked=None, keyframe=False, overlap=None).pruned == 0


def test_restatement_decides_in_float32():
    """One rounding per operation: a row whose float64 norm lies below scale_max and whose float32 norm does not; NaN is
    never kept; +inf switches the scale test off for finite norms only; the compaction is stable."""
    from prune_ref import compact, keep_mask, norm, opa_logit

    s = np.array([[0.1, 0.2, 0.3]], np.float32)
    n32 = norm(s, "abs")[0]
    n64 = math.sqrt(float(s[0, 0]) ** 2 + float(s[0, 1]) ** 2 + float(s[0, 2]) ** 2)
    want = np.sqrt(np.float32(np.float32(s[0, 0] * s[0, 0] + s[0, 1] * s[0, 1]) + s[0, 2] * s[0, 2]))
    assert n32 == want and n32.dtype == np.float32 and float(n32) != n64
    hi, lo = max(float(n32), n64), min(float(n32), n64)
    between = np.float32(hi)  # a threshold the two precisions see from different sides
    assert bool(keep_mask(s, [0.0], -1.0, between, "abs")[0]) == bool(n32 < between)
    assert lo < hi
    e = np.array([[0.5, -1.0, 2.0]], np.float32)
    assert norm(e, "exp")[0] == np.sqrt(np.float32(np.float32(np.exp(e[0, 0]) ** 2 + np.exp(e[0, 1]) ** 2) + np.exp(e[0, 2]) ** 2))
    nan = np.float32(np.nan)
    scale = np.array([[1, 1, 1], [nan, 1, 1], [1, 1, 1], [1, 1, 100], [1, 1, 1]], np.float32)
    opa = np.array([0.5, 0.5, nan, 0.5, -0.5], np.float32)
    assert keep_mask(scale, opa, 0.0, np.inf, "abs").tolist() == [True, False, False, True, False]
    assert keep_mask(scale, opa, 0.0, 50.0, "abs").tolist() == [True, False, False, False, False]
    assert keep_mask(scale, opa, 0.0, np.inf, "exp").tolist() == [True, False, False, False, False]  # exp(100) = inf: not < inf
    assert keep_mask(scale, [0.0] * 5, 0.0, np.inf, "abs").tolist() == [False] * 5  # opa equal to the threshold: not kept
    assert opa_logit(0.5) == 0.0 and opa_logit(0.02) == np.float32(-math.log(49.0))
    rows = np.arange(15, dtype=np.float32).reshape(5, 3)
    assert compact([rows, opa], np.array([True, False, False, True, True]))[0].tolist() == rows[[0, 3, 4]].tolist()


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


@pytest.mark.parametrize("part,vgprs", [("prune_classify_kernel", 15), ("prune_scan_kernel", 45), ("prune_apply_kernel", 34)])
def test_prune_kernels_are_small_and_free_of_scratch(kernels, part, vgprs):
    """Streaming kernels, eight waves per SIMD (64 VGPRs and fewer), no scratch: the apply kernel indexes its array table with a
    loop counter, and a copy of that table to scratch would be paid per array per workgroup.  The counts are the build's."""
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
    if part == "prune_apply_kernel":
        assert k[".group_segment_fixed_size"] == 1024  # the 256-entry rank -> row table and nothing else
