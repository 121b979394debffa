"""CPU tier of the per-Gaussian contributions (include/gs_abi.h: gs_frame_contrib_workspace_bytes, gs_frame_contrib,
gs_prune_classify_contrib): the symbols and their bindings, every refusal on fake pointers (each comes before anything is
enqueued), the workspace size query, the restatement (tests/contrib_ref.py) held against the oracle's alpha map and its own
monotonicity, the Python surface, and the scratch budget of the new kernels read from the built code objects.  No kernel is
launched."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_frame_contrib_workspace_bytes", "gs_frame_contrib", "gs_prune_classify_contrib"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for text in ("size_t gs_frame_contrib_workspace_bytes(", "int gs_frame_contrib(", "int gs_prune_classify_contrib(",
                 "} gs_contrib_row;", "} gs_contrib_opts;", "} gs_prune_contrib_opts;"):
        assert text in header
    assert _lib.lib.gs_abi_version() == 8 and "#define GS_ABI_VERSION 8" in header  # additive: the version stays
    assert C.sizeof(_lib.GsContribOpts) == 8 and C.sizeof(_lib.GsPruneContribOpts) == 12


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_frame_contrib_workspace_bytes
    sizes = [0, 1, 15, 16, 17, 50_000, 1 << 20, (1 << 30) - 1]
    got = [q(n) for n in sizes]
    for n, b in zip(sizes, got):
        assert b > 0 and b % 256 == 0 and b >= 16 * n
    assert got == sorted(got) and got[-1] > got[0]  # monotone
    assert got[-2] <= 16 * (1 << 20) + 1024          # one 16-byte row per pair and a header
    for bad in (-1, -(1 << 40)):
        assert q(bad) == 0


def test_frame_contrib_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib
    from gs_testutil import fake_frame

    ROWS, WS = FAKE + (10 << 30), FAKE + (11 << 30)

    def call(frame=None, opts="default", rows=ROWS, ws=WS, nbytes=None, w_min=1 / 255, accumulate=0):
        f = frame if frame is not None else fake_frame()
        o = _lib.GsContribOpts(w_min, accumulate) if opts == "default" else opts
        nb = _lib.gs_frame_contrib_workspace_bytes(f.max_pairs) if nbytes is None else nbytes
        return _lib.gs_frame_contrib(C.byref(f), C.byref(o) if o is not None else None, rows, ws, nb, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_frame_contrib" in msg and word in msg, (kw, msg)

    refused(b"training", frame=fake_frame(training=0))
    refused(b"rows", rows=None)
    refused(b"rows", rows=ROWS + 8)  # misaligned
    refused(b"opts", opts=None)
    for v in (math.nan, 0.0, -1.0, -0.0, 1.0000001, math.inf):
        refused(b"w_min", w_min=v)
    for a in (-1, 2, 7):
        refused(b"accumulate", accumulate=a)
    need = _lib.gs_frame_contrib_workspace_bytes(fake_frame().max_pairs)
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=need - 1)
    refused(b"workspace", nbytes=0)
    refused(b"workspace", ws=WS + 16)  # misaligned
    # every colour model and flag combination passes the same gate
    for kw in (dict(color_dim=27), dict(color_dim=48), dict(aux=True), dict(aux=True, color_dim=27)):
        refused(b"w_min", frame=fake_frame(**kw), w_min=0.0)
    # N = 0: valid, nothing to launch (rows may be null)
    assert call(frame=fake_frame(N=0), rows=None) == 0
    assert call(frame=fake_frame(N=0), w_min=1.0) == 0


def test_classify_contrib_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    N = 1000
    ws_bytes = _lib.gs_prune_workspace_bytes(N)
    SCALE, OPA, ROWS, CNT, WS = (FAKE + i * (1 << 24) for i in range(5))

    def popts(**kw):
        o = _lib.GsPruneOpts(-5.0, math.inf, 0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(scale=SCALE, opa=OPA, rows=ROWS, n=N, opts="default", copts="default", cnt=CNT, ws=WS, nbytes=ws_bytes):
        o = popts() if opts == "default" else opts
        c = _lib.GsPruneContribOpts(0.0, 0, 0) if copts == "default" else copts
        return _lib.gs_prune_classify_contrib(scale, opa, rows, n, C.byref(o) if o is not None else None,
                                              C.byref(c) if c is not None else None, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_prune_classify_contrib" in msg and word in msg, (kw, msg)

    # gs_prune_classify's refusals (tests/test_prune_host.py)
    refused(b"null", scale=None)
    refused(b"null", opa=None)
    refused(b"null", cnt=None)
    refused(b"null", opts=None)
    for n in (-1, -1000, 1 << 31):
        refused(b"N out of range", n=n, nbytes=1 << 40)
    for v in (math.inf, -math.inf, math.nan):
        refused(b"opa_logit_min", opts=popts(opa_logit_min=v))
    refused(b"scale_max", opts=popts(scale_max=math.nan))
    for act in (-1, 2, 7):
        refused(b"scale_activation", opts=popts(scale_activation=act))
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", ws=WS + 4)
    # ... and its own
    refused(b"null", rows=None)
    refused(b"null", copts=None)
    for v in (math.nan, -1e-9, -math.inf):
        refused(b"weight_max_min", copts=_lib.GsPruneContribOpts(v, 0, 0))


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def oracle_frame():
    from gs_scene import make_camera, make_scene
    from gs_testutil import OracleFrame

    scene = make_scene(300, 70, 45, seed=11)
    return OracleFrame(scene, make_camera(70, 45, yaw_deg=1.0))


def test_restatement_sums_to_the_oracles_alpha_map(oracle_frame):
    """sum_g w_g(p) is the alpha the oracle's K7 composites: drawn with every colour 1, its image IS that sum."""
    import oracle
    from contrib_ref import from_oracle_frame

    of = oracle_frame
    ref = from_oracle_frame(of)
    grid, rays = of.grid, of.rays
    ones = np.ones((len(of.ids), 3), np.float32)
    alpha = oracle.draw(of.s_pos, ones, of.s_opa, of.s_cov, of.accum, grid.padded_height, grid.padded_width, grid.focal_x,
                        grid.focal_y, use_sh=False, fast=True, rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx,
                        vdy=rays.dy)[:, :, 0]
    err = float(np.abs(ref.alpha_map.numpy() - alpha).max())
    print(f"restatement against the oracle's alpha map: max |diff| {err:.3e}")
    assert len(of.ids) > 300 and err <= 5e-5
    # the statistics are the sums of w over the cropped image
    crop = grid.crop(ref.alpha_map.numpy()[:, :, None])[:, :, 0]
    assert crop.shape == (45, 70)
    assert abs(float(ref.weight_sum.sum()) - float(crop.sum())) <= 1e-9 * max(1.0, float(crop.sum()))
    assert bool((ref.weight_max <= ref.weight_sum + 1e-15).all()) and bool((ref.views == (ref.pixels > 0)).all())
    culled = ~np.asarray(of.mask, bool)
    assert culled.any() and not ref.weight_sum.numpy()[culled].any() and not ref.pixels.numpy()[culled].any()


def test_restatement_is_monotone_in_stop_and_w_min(oracle_frame):
    from contrib_ref import from_oracle_frame

    of = oracle_frame
    prev = None
    for stop in (1e-1, 1e-2, 1e-4, 1e-6):  # a later stop composites more
        r = from_oracle_frame(of, stop=stop)
        if prev is not None:
            assert bool((r.weight_sum >= prev.weight_sum).all()) and bool((r.weight_max >= prev.weight_max).all())
            assert bool((r.pixels >= prev.pixels).all()) and bool((r.w >= prev.w).all())
        prev = r
    assert float(prev.weight_sum.sum()) > float(from_oracle_frame(of, stop=1e-1).weight_sum.sum())
    prev = None
    for w_min in (1e-4, 1 / 255, 0.05, 0.5):  # a higher floor counts fewer pixels and moves nothing else
        r = from_oracle_frame(of, w_min=w_min)
        if prev is not None:
            assert bool((r.pixels <= prev.pixels).all()) and bool((r.views <= prev.views).all())
            assert bool((r.weight_sum == prev.weight_sum).all()) and bool((r.weight_max == prev.weight_max).all())
        prev = r
    lo, hi = from_oracle_frame(of, w_min=1e-4), prev
    assert int(hi.pixels.sum()) < int(lo.pixels.sum())


# ------------------------------------------------------------------------------------------------------ Python surface
def test_python_surface_and_refusals():
    import torch

    import gs_frame
    import gs_prune
    import gs_slam
    import gs_train

    assert gs_frame.CONTRIB_W_MIN == 1.0 / 255.0
    sig = inspect.signature(gs_frame.FrameRenderer.contributions)
    assert list(sig.parameters) == ["self", "w_min", "out", "accumulate"]
    assert sig.parameters["w_min"].default == 1.0 / 255.0 and sig.parameters["out"].default is None
    assert sig.parameters["accumulate"].default is False
    c = gs_frame.Contributions(torch.zeros(5, 4), 1 / 255)
    c.rows.view(torch.int32)[:, 2] = torch.arange(5, dtype=torch.int32)
    c.rows[:, 1] = 0.25
    assert c.weight_sum.shape == (5,) and c.weight_max.tolist() == [0.25] * 5 and c.pixels.tolist() == [0, 1, 2, 3, 4]
    assert c.pixels.dtype == torch.int32 and c.views.dtype == torch.int32 and c.weight_sum.dtype == torch.float32
    assert c.pixels.data_ptr() == c.rows.data_ptr() + 8 and c.views.data_ptr() == c.rows.data_ptr() + 12  # views, not copies
    # contributions() before a forward (a renderer that never rendered: built without a device)
    r = object.__new__(gs_frame.FrameRenderer)
    r._frame = None
    with pytest.raises(RuntimeError, match="training forward"):
        r.contributions()
    # Trainer.contributions under view parallelism
    tr = object.__new__(gs_train.Trainer)
    tr.world_size = 2
    with pytest.raises(RuntimeError, match="world_size"):
        tr.contributions()
    sig = inspect.signature(gs_train.Trainer.contributions)
    assert list(sig.parameters) == ["self", "camera_ids", "w_min"] and sig.parameters["w_min"].default == 1.0 / 255.0
    sig = inspect.signature(gs_train.Trainer.prune)
    for name in ("opa_min", "scale_max", "contributions", "weight_max_min", "pixels_min", "views_min", "carry_state"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig.parameters["contributions"].default is None and sig.parameters["views_min"].default == 0
    assert sig.parameters["weight_max_min"].default == 0.0 and sig.parameters["pixels_min"].default == 0
    sig = inspect.signature(gs_prune.prune_rows)
    for name, default in (("contributions", None), ("weight_max_min", 0.0), ("pixels_min", 0), ("views_min", 0)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default == default
    so = gs_slam.SlamOptions()
    assert so.prune_unseen_every == 0 and so.prune_unseen_w_min == 1.0 / 255.0
    assert gs_slam.SlamFrame(rot=None, tran=None, tracked=None, keyframe=False, overlap=None).pruned_unseen == 0
    o = gs_prune.contrib_options(0.05, 3, 1)
    assert (o.weight_max_min, o.pixels_min, o.views_min) == (np.float32(0.05), 3, 1)
    for bad in (dict(weight_max_min=math.nan), dict(weight_max_min=-0.1), dict(pixels_min=-1), dict(views_min=-2)):
        with pytest.raises(ValueError):
            gs_prune.contrib_options(**bad)


def test_prune_without_contributions_issues_the_calls_it_issued(monkeypatch):
    """prune_rows / Trainer.prune without ``contributions``: gs_prune_classify with the option struct of before, never the new
    entry point; with them: the new entry point, the same gs_prune_opts, the thresholds in gs_prune_contrib_opts."""
    import torch

    import gs_prune
    import gs_train
    from gaussian import _lib

    calls = []

    class Stop(Exception):
        pass

    def fake(name):
        def f(*args):
            structs = [a._obj for a in args if hasattr(a, "_obj")]
            calls.append((name, [(type(s).__name__, [getattr(s, k) for k, _ in s._fields_]) for s in structs]))
            raise Stop

        return f

    monkeypatch.setattr(_lib, "gs_prune_classify", fake("gs_prune_classify"))
    monkeypatch.setattr(_lib, "gs_prune_classify_contrib", fake("gs_prune_classify_contrib"))
    monkeypatch.setattr(gs_prune, "_rows", lambda name, t, n=None: int(math.prod(t.shape[1:])))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **{**k, "device": "cpu"}))
    monkeypatch.setattr(torch, "zeros", (lambda z: lambda *a, **k: z(*a, **{**k, "device": "cpu"}))(torch.zeros))

    class Stream:
        cuda_stream = None

    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: Stream())

    class Dev:
        type = "cuda"

    class T:  # a stand-in for a HIP tensor: shape, device, address
        def __init__(self, *shape):
            self.shape, self.device = shape, Dev()

        def data_ptr(self):
            return FAKE

    scale, opa, rows = T(8, 3), T(8), T(8, 4)
    want = gs_prune.prune_options(0.01, 0.7, "exp")
    fields = lambda s: [getattr(s, k) for k, _ in s._fields_]  # noqa: E731
    with pytest.raises(Stop):
        gs_prune.prune_rows(scale, opa, [scale], opa_min=0.01, scale_max=0.7, scale_activation="exp")
    assert calls == [("gs_prune_classify", [("GsPruneOpts", fields(want))])]
    calls.clear()
    with pytest.raises(Stop):
        gs_prune.prune_rows(scale, opa, [scale], opa_min=0.01, scale_max=0.7, scale_activation="exp", contributions=rows,
                            weight_max_min=0.05, pixels_min=2, views_min=1)
    assert calls == [("gs_prune_classify_contrib", [("GsPruneOpts", fields(want)),
                                                    ("GsPruneContribOpts", [np.float32(0.05), 2, 1])])]
    with pytest.raises(ValueError):
        gs_prune.prune_rows(scale, opa, [scale], opa_min=0.01, views_min=1)
    # Trainer.prune: opa_min stays required without contributions; None with them = the most negative finite logit
    calls.clear()
    tr = object.__new__(gs_train.Trainer)
    tr.scale_activation = "abs"

    class Opt:
        sharded = False

    class Flat:
        params, n = [None, None, scale, opa, None], 8

        def finish_gather(self):
            pass

    tr.optimizer, tr.world_size, tr.view_stat, tr.grad_counter, tr.flat = Opt(), 1, None, None, Flat()
    with pytest.raises(TypeError):
        tr.prune(0)
    with pytest.raises(ValueError):
        tr.prune(0, opa_min=0.005, views_min=1)
    with pytest.raises(Stop):
        tr.prune(0, opa_min=0.005)
    assert calls == [("gs_prune_classify", [("GsPruneOpts", fields(gs_prune.prune_options(0.005, math.inf, "abs")))])]
    calls.clear()
    with pytest.raises(Stop):
        tr.prune(0, contributions=rows, views_min=1)
    (name, structs), = calls
    assert name == "gs_prune_classify_contrib" and structs[1] == ("GsPruneContribOpts", [0.0, 0, 1])
    assert structs[0][1][0] == -np.finfo(np.float32).max and structs[0][1][1] == math.inf


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


@pytest.mark.parametrize("part", ["contrib_pair_kernel", "contrib_gaussian_kernel", "prune_classify_contrib_kernel"])
def test_contrib_kernels_use_no_scratch(kernels, part):
    """Read from the code-object metadata alone.  The pair kernel keeps its per-(Gaussian, pixel) state in registers over the
    sixteen pixel rows of a tile: a spill would be paid per row step.  128 VGPRs and fewer: four waves per SIMD."""
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    print(part, "vgprs", k[".vgpr_count"], "sgprs", k[".sgpr_count"], "lds", k[".group_segment_fixed_size"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, (k[".name"], k[".vgpr_spill_count"])
    assert k[".vgpr_count"] <= 128
    if part == "contrib_pair_kernel":
        assert k[".group_segment_fixed_size"] <= 2048  # the tile's 256 transmittances and 16 row coordinates per wave
