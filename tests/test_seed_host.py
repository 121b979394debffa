"""CPU tier of seeding from RGB-D frames (include/gs_abi.h: gs_seed_workspace_bytes, gs_seed_classify, gs_seed_apply): the
symbols and their ctypes bindings, the workspace size query, every refusal on fake pointers (each comes before anything is
enqueued), the Python surface's defaults, the float32 restatement's lattice against the definition, and the register /
scratch budgets of the new kernels read from the built code objects.  No kernel is launched."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 96, 128


def _opts(**kw):
    from gaussian import _lib

    o = _lib.GsSeedOpts(1, 0.5, 0.2, 0.7, 0.9, 0, 3)
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

    for name in ("gs_seed_workspace_bytes", "gs_seed_classify", "gs_seed_apply"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_seed_workspace_bytes(", "int gs_seed_classify(", "int gs_seed_apply(", "} gs_seed_opts;",
                 "} gs_seed_camera;"):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays
    assert C.sizeof(_lib.GsSeedOpts) == 28 and C.sizeof(_lib.GsSeedCamera) == 64  # the header's layouts


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_seed_workspace_bytes
    sizes = [(1, 1), (48, 64), (187, 250), (480, 640), (1080, 1920), (2160, 3840)]
    got = [q(h, w) for h, w in sizes]
    for b in got:
        assert b > 0 and b % 256 == 0
    assert got == sorted(got) and got[-1] > got[0]  # monotone in H * W
    assert q(64, 48) == q(48, 64)  # ... and a function of H * W alone
    # a 64-bit ballot per 64 pixels and a count pair per 256: an eighth of a byte and a thirty-second per pixel
    assert 1080 * 1920 * (1 / 8 + 1 / 32) <= got[4] <= 1080 * 1920 * (1 / 8 + 1 / 32) + 1024
    for bad in ((-1, 64), (48, -7), (-3, -3)):
        assert q(*bad) == 0


def test_classify_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_seed_workspace_bytes(H, W)
    Z, D, A, CNT, WS = (FAKE + i * (1 << 24) for i in range(5))

    def call(rng=Z, depth=D, alpha=A, h=H, w=W, opts="default", cnt=CNT, ws=WS, nbytes=ws_bytes):
        o = _opts() if opts == "default" else opts
        return _lib.gs_seed_classify(rng, depth, alpha, h, w, C.byref(o) if o is not None else None, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_seed_classify" in msg or b"seed_check_opts" in msg, msg
        assert word in msg, (kw, msg)

    refused(b"null", rng=None)
    refused(b"null", cnt=None)
    refused(b"null", opts=None)
    refused(b"both or neither", depth=None)  # the maps given singly
    refused(b"both or neither", alpha=None)
    for s in (0, -1, -64):
        refused(b"stride", opts=_opts(stride=s))
    for cd in (0, 1, 4, 9, 16, 26, 49):
        refused(b"color_dim", opts=_opts(color_dim=cd))
    for act in (-1, 2):
        refused(b"scale_activation", opts=_opts(scale_activation=act))
    for p in (0.0, 1.0, -0.2, 1.5, float("nan")):
        refused(b"opa_init", opts=_opts(opa_init=p))
    for f in (0.0, -1.0, float("inf"), float("nan")):
        refused(b"scale_factor", opts=_opts(scale_factor=f))
    refused(b"finite", opts=_opts(alpha_thresh=float("nan")))
    refused(b"finite", opts=_opts(front_rel=float("inf")))
    for hw in ((-1, W), (H, -5), (0, W), (H, 0), (1 << 16, 1 << 16)):
        refused(b"size", h=hw[0], w=hw[1])
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"workspace", ws=WS + 4)


def test_apply_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_seed_workspace_bytes(H, W)
    IMG, Z, CNT, WS, POS, QUAT, SCALE, OPA, RGB = (FAKE + i * (1 << 24) for i in range(9))

    def call(image=IMG, rng=Z, cam="default", opts="default", pos=POS, quat=QUAT, scale=SCALE, opa=OPA, rgb=RGB, offset=0,
             capacity=1000, cnt=CNT, ws=WS, nbytes=ws_bytes):
        o = _opts() if opts == "default" else opts
        c = _cam() if cam == "default" else cam
        return _lib.gs_seed_apply(image, rng, C.byref(c) if c is not None else None, C.byref(o) if o is not None else None,
                                  pos, quat, scale, opa, rgb, offset, capacity, cnt, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_seed_apply" in msg or b"seed_check_opts" in msg, msg
        assert word in msg, (kw, msg)

    for kw in ("image", "rng", "cam", "opts", "cnt", "pos", "quat", "scale", "opa", "rgb"):
        refused(b"null", **{kw: None})
    refused(b"stride", opts=_opts(stride=0))
    refused(b"color_dim", opts=_opts(color_dim=12))
    refused(b"negative", offset=-1)
    refused(b"negative", capacity=-1)
    refused(b"size", cam=_cam(width=-4))
    refused(b"size", cam=_cam(height=0))
    refused(b"focal", cam=_cam(focal_x=0.0))
    refused(b"focal", cam=_cam(focal_y=float("nan")))
    refused(b"workspace", ws=None)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"aligned", quat=QUAT + 4)
    # arrays that are already full take no row: nothing to launch, nothing to complain about
    assert call(offset=1000, capacity=1000) == 0 and call(offset=5, capacity=0) == 0


def test_python_surface_and_defaults():
    import gs_seed
    import gs_train

    sig = inspect.signature(gs_seed.seed_from_depth)
    assert list(sig.parameters)[:3] == ["image", "depth", "camera"]
    for name in ("rendered", "depth_kind", "stride", "alpha_thresh", "front_rel", "scale_factor", "opa_init", "color_dim",
                 "scale_activation", "append_to"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["rendered"] is None and d["append_to"] is None and d["depth_kind"] == "range" and d["stride"] == 1
    assert d["color_dim"] == 3 and d["scale_activation"] == "abs"
    # a seeded pixel has A >= opa_init at its centre: it must not be selected again
    assert 0.0 < d["alpha_thresh"] < d["opa_init"] < 1.0 and 0.0 < d["front_rel"] < 1.0 and d["scale_factor"] > 0.0
    o = gs_seed.seed_options()
    assert (o.stride, o.scale_activation, o.color_dim) == (1, 0, 3)
    assert gs_seed.seed_options(scale_activation="exp", color_dim=48, stride=3).scale_activation == 1
    sig = inspect.signature(gs_train.Trainer.seed_from_view)
    assert list(sig.parameters)[:3] == ["self", "camera_id", "i_iter"]
    assert list(sig.parameters.values())[-1].kind is inspect.Parameter.VAR_KEYWORD
    import torch

    with pytest.raises(RuntimeError):  # a HIP kernel: no CPU fallback
        gs_seed.seed_from_depth(torch.zeros(4, 4, 3), torch.ones(4, 4), None)
    with pytest.raises(ValueError):
        gs_seed.seed_from_depth(torch.zeros(4, 4, 3), torch.ones(4, 4), None, depth_kind="disparity")


@pytest.mark.parametrize("stride", [1, 2, 3, 5, 16])
def test_restatement_lattice_is_the_definition(stride):
    """x % stride == stride // 2 and y % stride == stride // 2, in row-major order."""
    from seed_ref import lattice

    for Hh, Ww in ((1, 1), (7, 9), (48, 64), (187, 250)):
        ys, xs = lattice(Hh, Ww, stride)
        want = [(y, x) for y in range(Hh) for x in range(Ww) if x % stride == stride // 2 and y % stride == stride // 2]
        assert list(zip(ys.tolist(), xs.tolist())) == want


def test_restatement_decides_in_float32():
    """One rounding per operation: a case where float64 and float32 disagree about z A < (1 - front_rel) D."""
    from seed_ref import select

    z = np.array([[np.float32(3.0000002)]], np.float32)
    A = np.array([[np.float32(0.9)]], np.float32)
    keep = np.float32(1.0) - np.float32(0.1)
    D = np.array([[np.float32(z[0, 0] * A[0, 0]) / keep]], np.float32)
    sel, meas = select(z, D, A, stride=1, alpha_thresh=0.5, front_rel=0.1)
    want = np.float32(z[0, 0] * A[0, 0]) < np.float32(keep * D[0, 0])
    assert meas.tolist() == [[True]] and bool(sel[0, 0]) == bool(want)
    for bad in (0.0, -1.0, np.inf, np.nan):
        sel, meas = select(np.array([[bad]], np.float32), None, None, 1, 0.5, 0.1)
        assert not sel.any() and not meas.any()


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


@pytest.mark.parametrize("part,vgprs", [("seed_classify_kernel", 32), ("seed_scan_kernel", 72), ("seed_apply_kernelILi3E", 48),
                                        ("seed_apply_kernelILi27E", 48), ("seed_apply_kernelILi48E", 48)])
def test_seed_kernels_are_small_and_free_of_scratch(kernels, part, vgprs):
    """Streaming kernels: eight waves per SIMD (64 VGPRs) for the two that touch the maps, no scratch anywhere -- the SH
    variant's row walk is a loop, and a spill in it would be paid per float."""
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0
