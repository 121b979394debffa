"""CPU tier of coarse-to-fine tracking (include/gs_abi.h: gs_pyramid_down; gs_pyramid.Pyramid / level_camera;
gs_track.TrackOptions.pyramid): the symbol and its binding, every refusal on fake pointers (each comes before anything is
enqueued), the float32 restatement (tests/pyramid_ref.py) against a float64 mean, the level cameras against the pinhole
relation and the renderer's own ray basis, the schedule's validation, and the resources of the two kernel instantiations read
from the built code object.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import pyramid_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 48, 64


def test_symbol_exists_and_is_bound():
    from gaussian import _lib

    assert "gs_pyramid_down" in _lib.EXPORTS
    assert getattr(_lib.lib, "gs_pyramid_down") is not None and callable(_lib.gs_pyramid_down)
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    assert "int gs_pyramid_down(" in header and "typedef struct gs_pyramid_opts {" in header
    assert "#define GS_PYRAMID_MAX_LEVELS 4" in header and _lib.GS_PYRAMID_MAX_LEVELS == 4
    assert C.sizeof(_lib.GsPyramidOpts) == 8
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays
    assert "#define GS_ABI_VERSION 8" in header
    import gs_build

    assert "-ffp-contract=off" in gs_build.SOURCES["pyramid.hip"]  # one rounding per operation: the contract


def test_down_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    IMG, RNG, OUT, ROUT = (FAKE + i * (1 << 28) for i in range(4))

    def call(image=IMG, rng=RNG, h=H, w=W, opts=(2, 0.1), out=OUT, rout=ROUT):
        o = C.byref(_lib.GsPyramidOpts(*opts)) if opts is not None else None
        return _lib.gs_pyramid_down(image, rng, h, w, o, out, rout, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_pyramid_down" in msg and word in msg, (kw, msg)

    refused(b"image", image=None)
    refused(b"image_out", out=None)
    refused(b"opts", opts=None)
    refused(b"range and range_out", rng=None)       # one of the two given
    refused(b"range and range_out", rout=None)
    for hw in ((0, W), (H, 0), (-2, W), (H, -4), (H + 1, W), (H, W - 1), (1, 1)):
        refused(b"H and W", h=hw[0], w=hw[1])
    for kw, base, word in (("image", IMG, b"image must"), ("rng", RNG, b"range must"), ("out", OUT, b"image_out must"),
                           ("rout", ROUT, b"range_out must")):
        for off in (4, 8, 12):
            refused(word + b" be 16-byte aligned", **{kw: base + off})
    for mv in (0, 5, -1):
        refused(b"min_valid", opts=(mv, 0.1))
    refused(b"edge_rel", opts=(2, float("nan")))
    n_in, n_out = H * W * 4, (H // 2) * (W // 2) * 4
    # an output that starts inside an input, one that ends inside it, and the same buffer; then the first byte behind is fine
    for kw in ({"out": IMG}, {"out": IMG + 3 * n_in - 16}, {"out": IMG - 3 * n_out + 16}, {"out": RNG + 16}, {"rout": IMG + 64},
               {"rout": RNG}, {"rout": RNG + n_in - 16}, {"rout": RNG - n_out + 16}):
        refused(b"overlaps", **kw)
    refused(b"overlaps", rng=None, rout=None, out=IMG + 32)  # RGB only: the colour pair is still checked
    assert b"invalid argument" in _lib.gs_last_error()


def _f64_mean(rng):
    z = [rng[0::2, 0::2], rng[0::2, 1::2], rng[1::2, 0::2], rng[1::2, 1::2]]
    m = [pyramid_ref.measured(v) for v in z]
    n = sum(mk.astype(np.int64) for mk in m)
    s = sum(np.where(mk, zk, 0.0).astype(np.float64) for mk, zk in zip(m, z))
    return s / np.maximum(n, 1), n


@pytest.mark.parametrize("shape", [(22, 36), (120, 160)])
def test_restatement_against_a_float64_mean(shape):
    """Colour: three additions of non-negative numbers and an exact product; range: three additions and a division -- at most
    four roundings of 2^-24 relative each: within 2^-22 of the float64 mean on the measured pixels.  The measured set itself
    is restated independently: n >= min_valid and max <= fl(1.1f) min in float32."""
    image, rng = pyramid_ref.inputs(*shape, seed=11)
    out, rout = pyramid_ref.down(image, rng, 2, 0.1)
    assert out.dtype == np.float32 and rout.dtype == np.float32 and out.shape == (shape[0] // 2, shape[1] // 2, 3)
    i64 = image.astype(np.float64)
    mean = (i64[0::2, 0::2] + i64[0::2, 1::2] + i64[1::2, 0::2] + i64[1::2, 1::2]) / 4
    assert np.all(np.abs(out - mean) <= 2.0 ** -22 * np.abs(mean))
    want, n = _f64_mean(rng)
    got_m = rout > 0
    assert np.all(np.abs(rout - want)[got_m] <= 2.0 ** -22 * want[got_m])
    assert np.all(rout[~got_m] == 0) and not np.signbit(rout[~got_m]).any()  # exactly +0.0
    assert 0.2 < got_m.mean() < 0.95 and (n[got_m] >= 2).all() and (n == 0).any() and (n == 4).any()
    off = pyramid_ref.down(image, rng, 2, -1.0)[1]
    assert np.array_equal(off > 0, n >= 2) and (off > 0).sum() > got_m.sum()  # the edge test cuts some footprints
    # the crafted footprints: (0, j) has j measured pixels; (1, 0) sits exactly on the edge bound, (1, 1) one float above
    for j in range(5):
        assert n[0, j] == j and (rout[0, j] == (3.0 if j >= 2 else 0.0))
    assert rout[1, 0] > 0 and rout[1, 1] == 0 and off[1, 1] > 0
    assert pyramid_ref.down(image, rng, 2, 0.0)[1][1, 0] == 0  # edge_rel 0: only equal ranges count
    for mv in (1, 2, 3, 4):
        assert np.array_equal(pyramid_ref.down(image, rng, mv, -1.0)[1] > 0, n >= mv)


def test_level_two_is_down_after_down_and_the_sizes():
    import gs_pyramid

    image, rng = pyramid_ref.inputs(24, 40, seed=5)
    a = pyramid_ref.level(image, rng, 2)
    b = pyramid_ref.down(*pyramid_ref.down(image, rng))
    assert a[0].shape == (6, 10, 3) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert pyramid_ref.level(image, rng, 0)[0] is image
    assert pyramid_ref.level(image, None, 2)[1] is None
    assert gs_pyramid.level_sizes(24, 40, 2) == [(24, 40), (12, 20), (6, 10)]
    assert gs_pyramid.level_sizes(24, 40, 0) == [(24, 40)]
    with pytest.raises(ValueError, match="40 x 24 frame has no level 4"):
        gs_pyramid.level_sizes(24, 40, 4)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="GS_PYRAMID_MAX_LEVELS"):
            gs_pyramid.level_sizes(32, 32, bad)
    with pytest.raises(ValueError, match="has no level 1"):
        gs_pyramid.Pyramid(31, 32, 1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gs_pyramid.Pyramid(32, 32, 1, "cpu")
    doc = gs_pyramid.Pyramid.__doc__
    assert "no evidence" in doc and "arbitrary" in doc


# ----------------------------------------------------------------------------------------------------- level cameras
def _cameras():
    from gs_scene import make_camera
    from gs_testutil import general_camera

    even = make_camera(64, 32)
    odd = general_camera(60, 44)           # a rotated, shifted camera with fx != fy: 15 x 11 at level 2
    off = general_camera(60, 44)
    off.cx, off.cy = 33.25, 20.5
    return {"even": even, "odd": odd, "off": off}


def _pixel_point(cam, u, v):
    """The world point on the image plane z = 1 that pixel COORDINATE (u, v) of ``cam`` looks at, from the renderer's own ray
    basis (gs_geometry.RayBasis on the padded grid, the principal point's offset taken where the renderer takes it)."""
    from gs_geometry import RayBasis, TileGrid, principal_point_offset

    g = TileGrid(cam.width, cam.height, cam.focal_x, cam.focal_y)
    top, left = g.crop_offsets()
    rb = RayBasis.from_camera(cam.rot, cam.tran, g.padded_height, g.padded_width, cam.focal_x, cam.focal_y,
                              principal_point_offset(cam))
    # lefttop is the centre of padded pixel (0, 0), i.e. coordinate (0.5, 0.5) of the padded grid
    return (rb.lefttop.astype(np.float64) + (u + left - 0.5) * rb.dx.astype(np.float64)
            + (v + top - 0.5) * rb.dy.astype(np.float64))


@pytest.mark.parametrize("name,levels", [("even", (1, 2, 3, 4)), ("odd", (1, 2)), ("off", (1, 2))])
def test_level_camera_is_the_exact_pinhole_relation(name, levels):
    from gs_geometry import principal_point_default, principal_point_offset
    from gs_pyramid import level_camera

    cam = _cameras()[name]
    before = dict(vars(cam))
    assert level_camera(cam, 0) is cam and (name == "off" or cam.cx is None)  # level 0: unchanged, no cx gained
    cx0, cy0 = principal_point_default(cam.width, cam.height)
    cx = cx0 if cam.cx is None else cam.cx
    cy = cy0 if cam.cy is None else cam.cy
    rng = np.random.default_rng(3)
    P = np.stack([rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50), rng.uniform(1, 5, 50)], 1)  # camera space
    u, v = cam.focal_x * P[:, 0] / P[:, 2] + cx, cam.focal_y * P[:, 1] / P[:, 2] + cy
    for l in levels:
        c = level_camera(cam, l)
        assert c is not cam and (c.width, c.height) == (cam.width >> l, cam.height >> l)
        assert c.rot is cam.rot and c.tran is cam.tran and c.near == cam.near
        ul, vl = c.focal_x * P[:, 0] / P[:, 2] + c.cx, c.focal_y * P[:, 1] / P[:, 2] + c.cy
        # (a power of two scales exactly: what is left are the roundings of the two sums)
        assert np.all(np.abs(ul * 2 ** l - u) <= 4 * np.finfo(np.float64).eps * (np.abs(u) + cx))
        assert np.all(np.abs(vl * 2 ** l - v) <= 4 * np.finfo(np.float64).eps * (np.abs(v) + cy))
        dx, dy = principal_point_offset(c)
        if name == "even":
            assert (dx, dy) == (0.0, 0.0)
        elif name == "odd" and l == 2:
            assert (c.width, c.height) == (15, 11) and (dx, dy) == (-0.5, -0.5)
        # the centre ray of level pixel (i, j) is the fine camera's ray through (2^l (i + 1/2), 2^l (j + 1/2)); the basis is
        # float32 with entries of order 1 and pixel indices up to 64: 1e-5 is a few dozen of its roundings, and a half-pixel
        # convention error would be 2^(l-1) / focal >= 0.01
        for i, j in ((0, 0), (c.width - 1, 0), (0, c.height - 1), (c.width // 2, c.height // 3), (c.width - 1, c.height - 1)):
            a = _pixel_point(c, i + 0.5, j + 0.5)
            b = _pixel_point(cam, 2 ** l * (i + 0.5), 2 ** l * (j + 0.5))
            assert np.abs(a - b).max() <= 1e-5, (name, l, i, j, a, b)
            wrong = _pixel_point(cam, 2 ** l * (i + 0.5) + 2 ** (l - 1), 2 ** l * (j + 0.5))
            assert np.abs(a - wrong).max() > 5e-3
    assert dict(vars(cam)) == before  # the camera handed in is never written
    with pytest.raises(ValueError):
        level_camera(cam, 5)
    if name != "even":
        with pytest.raises(ValueError, match="has no level 3"):
            level_camera(cam, 3)  # 60 x 44


# ------------------------------------------------------------------------------------------------------ the schedule
def test_schedule_validation_needs_no_device():
    import gs_track

    T = gs_track.TrackOptions
    assert T().pyramid == () and T().stages() == () and gs_track.Tracker.level_plan(T(), 120, 160) is None
    ok = T(pyramid=((2, 100), (1, 100), (0, 100)))
    assert ok.stages() == ((2, 100), (1, 100), (0, 100))
    assert gs_track.Tracker.level_plan(ok, 120, 160) == [(2, 30, 40), (1, 60, 80), (0, 120, 160)]
    assert gs_track.Tracker.level_plan(T(pyramid=[[3, 5], [1, 7]]), 120, 160) == [(3, 15, 20), (1, 60, 80)]
    for bad, word in ((((1, 10), (1, 10)), "strictly decreasing"), (((0, 10), (1, 10)), "strictly decreasing"),
                      (((-1, 10),), "outside 0..4"), (((5, 10), (0, 10)), "outside 0..4"), (((1, 0),), "at least 1"),
                      (((2, 10), (0, -3)), "at least 1"), (((1, 2, 3),), "pairs"), (((1.5, 2),), "pairs")):
        with pytest.raises(ValueError, match=word):
            T(pyramid=bad).stages()
        with pytest.raises(ValueError, match=word):
            gs_track.Tracker.level_plan(T(pyramid=bad), 128, 128)
    # a size the deepest level does not divide: named with the level
    for (h, w), sched in (((120, 162), ((2, 10), (0, 10))), ((44, 60), ((3, 10),)), ((121, 160), ((1, 10),))):
        with pytest.raises(ValueError, match=f"{w} x {h} frame cannot be tracked at pyramid level {sched[0][0]}"):
            gs_track.Tracker.level_plan(T(pyramid=sched), h, w)
    assert gs_track.Tracker.level_plan(T(pyramid=((2, 10), (0, 10))), 44, 60) == [(2, 11, 15), (0, 44, 60)]
    names = list(T.__dataclass_fields__)
    assert names[-5:] == ["depth_gate_k", "color_gate_k", "depth_gate_floor", "color_gate_floor", "gate_couple"]
    assert names[-6] == "pyramid"  # in front of the gate's fields
    res = gs_track.TrackResult(rot=np.eye(3), tran=np.zeros(3), loss=0.0, iterations=0)
    assert res.levels is None and "levels" not in gs_track.TrackResult.__dataclass_fields__
    # the gate's plan is per level: the same class and arguments at the level's size
    g = T(pyramid=((1, 3), (0, 3)), depth_gate_k=10.0)
    assert gs_track.Tracker.loss_plan(g, 60, 80)[1][:2] == (60, 80) and gs_track.Tracker.loss_plan(g, 60, 80)[2] == 20


# -------------------------------------------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


@pytest.mark.parametrize("part", ["pyramid_down_kernelILb1EE", "pyramid_down_kernelILb0EE"])
def test_pyramid_kernels_have_no_scratch_and_no_lds(kernels, part):
    """csrc/pyramid.hip states: no LDS, no scratch; 256 lanes per workgroup.  A lane holds two fine rows of eight pixels (48
    colour floats) and its twelve outputs: at most 128 VGPRs, four waves per SIMD, is ample for a streaming kernel."""
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch
    assert k[".group_segment_fixed_size"] == 0, (k[".name"], k[".group_segment_fixed_size"])
    assert k[".vgpr_count"] <= 128, (k[".name"], k[".vgpr_count"])
    assert k[".max_flat_workgroup_size"] == 256


def test_no_pyramid_kernel_name_collides_with_a_pinned_one(kernels):
    """The tests that pick a kernel by a substring of its name demand exactly one hit: the new kernels add none."""
    import re

    import test_kernel_resources
    from test_track_gate_host import GATE_KERNELS
    from test_track_host import TRACK_KERNELS

    src = open(test_kernel_resources.__file__).read()
    pinned = set(re.findall(r'"([A-Za-z_0-9]*kernel[A-Za-z_0-9]*)"', src)) | set(TRACK_KERNELS) | set(GATE_KERNELS)
    new = [k for k in kernels if "pyramid_down" in k]
    assert len(new) == 2
    for k in new:
        assert not any(p in k for p in pinned), k
