"""CPU tier of the off-centre principal point (gs_scene.Camera.cx / cy; GS_FRAME_PRINCIPAL_POINT, gs_seed_apply_pp and
gs_view_overlap_pp of include/gs_abi.h): the offset helper and the struct sizes, gs_colmap.load_scene(principal_point=True),
the seeding ray and the overlap decision of csrc/overlap_point.h compiled for the host against the float32 restatements of
tests/pp_testutil.py, the z-depth conversion against its fp64 formula, and the refusals.  No kernel is launched."""
import copy
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import overlap_ref as R
import pp_testutil as P
from gs_geometry import RayBasis, principal_point_default, principal_point_offset
from gs_scene import Camera, make_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splatting_amd", "csrc")
GS_E_INVALID = -1


# ------------------------------------------------------------------------------------------------------- 1. the offset helper
def test_default_principal_point_and_zero_offsets():
    assert principal_point_default(128, 96) == (64.0, 48.0)
    assert principal_point_default(120, 90) == (60.0, 45.0)    # padded 128 x 96, crop left = 4, top = 3: 64 - 4, 48 - 3
    assert principal_point_default(121, 91) == (61.0, 46.0)    # odd: (W + 1) / 2 -- pad 128, left = 3: 64 - 3
    assert principal_point_default(1, 17) == (1.0, 9.0)
    for w, h in ((128, 96), (120, 90), (121, 91), (333, 201), (16, 16), (17, 15)):
        cam = make_camera(w, h)
        assert cam.cx is None and cam.cy is None
        assert principal_point_offset(cam) == (0.0, 0.0)
        cx0, cy0 = principal_point_default(w, h)
        assert cx0 == (w / 2 if w % 2 == 0 else (w + 1) / 2) and cy0 == (h / 2 if h % 2 == 0 else (h + 1) / 2)
        spelled = copy.copy(cam)
        spelled.cx, spelled.cy = cx0, cy0
        off = principal_point_offset(spelled)
        assert off == (0.0, 0.0) and all(np.signbit(v) == False for v in off)  # noqa: E712  (+0.0, not -0.0)
        half = copy.copy(cam)
        half.cx = cx0 + 2.5  # one coordinate given: the other keeps its default
        assert principal_point_offset(half) == (2.5, 0.0)
    # positional construction keeps working; the new fields trail `near`
    c = Camera(64, 48, 50.0, 51.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    assert (c.near, c.cx, c.cy) == (0.3, None, None)
    c = Camera(64, 48, 50.0, 51.0, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 0.2, 30.0, 25.5)
    assert (c.near, c.cx, c.cy) == (0.2, 30.0, 25.5) and principal_point_offset(c) == (-2.0, 1.5)
    # a camera-like object without the fields is a centred camera
    assert principal_point_offset(R._camera(53, 37, 40.0, 42.0, np.eye(3), np.zeros(3))) == (0.0, 0.0)
    bad = copy.copy(c)
    bad.cx = float("nan")
    with pytest.raises(ValueError):
        principal_point_offset(bad)


def test_ray_basis_with_a_zero_offset_is_the_ray_basis():
    cam = make_camera(121, 91, yaw_deg=7.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    a = RayBasis.from_camera(cam.rot, cam.tran, 96, 128, 90.75, 80.0)
    b = RayBasis.from_camera(cam.rot, cam.tran, 96, 128, 90.75, 80.0, pp_offset=(0.0, 0.0))
    for name in ("rays_o", "lefttop", "dx", "dy"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    c = RayBasis.from_camera(cam.rot, cam.tran, 96, 128, 90.75, 80.0, pp_offset=(7.3, -4.6))
    assert c.rays_o.tobytes() == a.rays_o.tobytes() and c.dx.tobytes() == a.dx.tobytes() and c.dy.tobytes() == a.dy.tobytes()
    # the corner ray moves by -(dx / fx, dy / fy) in camera coordinates: lefttop = c2w (lefttop_cam - tran)
    w2c = cam.rot.astype(np.float64)
    moved = w2c @ (c.lefttop.astype(np.float64) - a.lefttop.astype(np.float64))
    assert np.allclose(moved, [-7.3 / 90.75, 4.6 / 80.0, 0.0], atol=1e-6)


def test_struct_sizes_are_those_of_the_parent_commit():
    from gaussian import _lib

    assert C.sizeof(_lib.GsFrame) == 360 and C.sizeof(_lib.GsFrameScene) == 392 and C.sizeof(_lib.GsSeedCamera) == 64
    assert C.sizeof(_lib.GsFramePP) == 408 and _lib.GsFramePP.pp_dx.offset == 392 and _lib.GsFramePP.pp_dy.offset == 400
    assert C.sizeof(_lib.GsSeedCameraPP) == 72 and _lib.GsSeedCameraPP.pp_dx.offset == 64
    assert _lib.GS_FRAME_PRINCIPAL_POINT == 16384 and _lib.gs_abi_version() == 8
    text = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for piece in ("#define GS_FRAME_PRINCIPAL_POINT 16384", "} gs_frame_pp;", "} gs_seed_camera_pp;", "int gs_seed_apply_pp(",
                  "int gs_view_overlap_pp("):
        assert piece in text, piece


def test_frame_flag_validation_without_a_gpu():
    """The flag is accepted; an offset that is not finite is refused before anything is enqueued (the frame has fake pointers:
    a call that got past validation would fault, so only refusals are provoked here)."""
    from gaussian import _lib
    from gs_testutil import fake_frame

    base = fake_frame(training=0)
    f = _lib.GsFramePP()
    C.memmove(C.byref(f), C.byref(base), C.sizeof(_lib.GsFrame))
    f.flags |= _lib.GS_FRAME_PRINCIPAL_POINT
    for dx, dy in ((float("nan"), 0.0), (0.0, float("inf")), (2.0e6, 0.0)):
        f.pp_dx, f.pp_dy = dx, dy
        assert _lib.gs_frame_forward(C.byref(f), None) == GS_E_INVALID
        assert b"GS_FRAME_PRINCIPAL_POINT" in _lib.gs_last_error()
    f.pp_dx, f.pp_dy, f.focal_x = 1.0, 1.0, 0.0
    assert _lib.gs_frame_forward(C.byref(f), None) == GS_E_INVALID and b"focal" in _lib.gs_last_error()
    cam = _lib.GsSeedCameraPP()
    cam.cam.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    cam.cam.focal_x = cam.cam.focal_y = 96.0
    cam.cam.width, cam.cam.height = 128, 96
    cam.pp_dx = float("nan")
    opts = _lib.GsSeedOpts(1, 0.5, 0.2, 0.7, 0.9, 0, 3)
    FAKE = 1 << 40
    assert _lib.gs_seed_apply_pp(FAKE, FAKE, C.byref(cam), C.byref(opts), FAKE, FAKE, FAKE, FAKE, FAKE, 0, 10, FAKE, FAKE,
                                 1 << 20, None) == GS_E_INVALID
    assert b"principal point" in _lib.gs_last_error()
    oo = _lib.GsOverlapOpts(1, 0.3, 0)
    assert _lib.gs_view_overlap_pp(FAKE, C.byref(cam), FAKE, None, 1, C.byref(oo), FAKE, FAKE, 1 << 20, None) == GS_E_INVALID
    assert b"principal point" in _lib.gs_last_error()
    cam.pp_dx = 1.0
    assert _lib.gs_view_overlap_pp(FAKE, C.byref(cam), FAKE, FAKE + 4, 1, C.byref(oo), FAKE, FAKE, 1 << 20,
                                   None) == GS_E_INVALID  # view_pp_dev not 8-byte aligned
    assert b"view_pp_dev" in _lib.gs_last_error()


def test_splatter_refuses_a_principal_point():
    """The reference's class API is out of scope: intrinsics that carry cx / cy are refused, not ignored."""
    import splatter

    s = object.__new__(splatter.Splatter)  # (no dataset, no device: set_camera's refusal comes before it touches either)
    intr = {"width": 64, "height": 48, "focal_x": 50.0, "focal_y": 50.0}
    for extra in ({"cx": 30.0}, {"cy": 20.0}, {"cx": 32.0, "cy": 24.0}):
        with pytest.raises(RuntimeError, match="cx / cy"):
            s.set_camera(None, extrinsics={"rot": np.eye(3), "tran": np.zeros(3)}, intrinsics=dict(intr, **extra))


# ------------------------------------------------------------------------------------------------------------ 2. load_scene
def _capture(root, model, params, ds=2):
    import gs_colmap as gc
    from PIL import Image

    os.makedirs(os.path.join(root, "sparse", "0"))
    os.makedirs(os.path.join(root, f"images_{ds}"))
    cams = {1: gc.ColmapCamera(1, model, 64, 48, np.asarray(params, np.float64))}
    q = np.array([0.9, 0.1, -0.2, 0.3])
    imgs = {4: gc.ColmapImage(4, q / np.linalg.norm(q), np.array([0.1, 0.2, 0.3]), 1, "a.png", np.zeros((1, 2)),
                              np.array([-1], np.int64))}
    pts = {1: gc.ColmapPoint3D(1, np.zeros(3), np.array([1, 2, 3], np.uint8), 0.1, np.array([4], np.int32),
                               np.array([0], np.int32))}
    Image.fromarray(np.zeros((48 // ds, 64 // ds, 3), np.uint8), "RGB").save(os.path.join(root, f"images_{ds}", "a.png"))
    gc.write_cameras_binary(os.path.join(root, "sparse", "0", "cameras.bin"), cams)
    gc.write_images_binary(os.path.join(root, "sparse", "0", "images.bin"), imgs)
    gc.write_points3d_binary(os.path.join(root, "sparse", "0", "points3D.bin"), pts)


def test_load_scene_reads_the_principal_point_by_camera_model(tmp_path):
    import gs_colmap as gc

    _capture(str(tmp_path / "p"), "PINHOLE", [70.0, 72.0, 35.5, 21.0])
    _capture(str(tmp_path / "s"), "SIMPLE_PINHOLE", [90.0, 30.0, 26.5])
    _capture(str(tmp_path / "r"), "SIMPLE_RADIAL", [90.0, 30.0, 26.5, 0.01])
    cam = gc.load_scene(str(tmp_path / "p"), render_downsample=2, principal_point=True).cameras[0]
    assert (cam.width, cam.height, cam.focal_x, cam.focal_y, cam.cx, cam.cy) == (32, 24, 35.0, 36.0, 17.75, 10.5)
    assert principal_point_offset(cam) == (1.75, -1.5)
    cam = gc.load_scene(str(tmp_path / "s"), render_downsample=2, principal_point=True).cameras[0]
    assert (cam.focal_x, cam.focal_y, cam.cx, cam.cy) == (45.0, 45.0, 15.0, 13.25)
    with pytest.raises(RuntimeError, match="SIMPLE_RADIAL"):
        gc.load_scene(str(tmp_path / "r"), render_downsample=2, principal_point=True)
    # the default stays the reference's reading: params[0:2] whatever the model, no principal point
    for d, want in (("p", (35.0, 36.0)), ("s", (45.0, 15.0)), ("r", (45.0, 15.0))):
        cam = gc.load_scene(str(tmp_path / d), render_downsample=2).cameras[0]
        assert (cam.focal_x, cam.focal_y) == want and cam.cx is None and cam.cy is None
        assert principal_point_offset(cam) == (0.0, 0.0)


# ----------------------------------------------------------------------- 3. seeding ray and overlap decision, compiled for the host
_MAIN = r"""
#include <cstdio>
#include <vector>
#include "overlap_point.h"
int main() {
    int32_t hdr[3];  // n_views, n_points, border
    float near;
    gs_seed_camera_pp cam;
    if (fread(hdr, 4, 3, stdin) != 3 || fread(&near, 4, 1, stdin) != 1 || fread(&cam, 72, 1, stdin) != 1) return 2;
    std::vector<gs_seed_camera> views(hdr[0]);
    std::vector<float> pp(2 * hdr[0]);
    if (fread(views.data(), 64, hdr[0], stdin) != (size_t)hdr[0]) return 2;
    if (fread(pp.data(), 8, hdr[0], stdin) != (size_t)hdr[0]) return 2;
    for (int i = 0; i < hdr[1]; ++i) {
        int32_t xy[2];
        float z, p[3] = {0.f, 0.f, 0.f};
        if (fread(xy, 4, 2, stdin) != 2 || fread(&z, 4, 1, stdin) != 1) return 2;
        const bool m = gs_overlap_measured(z);
        if (m) gs_overlap_point_pp(cam.cam, cam.pp_dx, cam.pp_dy, xy[0], xy[1], z, p);
        fwrite(p, 4, 3, stdout);
        for (int k = 0; k < hdr[0]; ++k)
            putchar(m && gs_overlap_seen_pp(p, views[k], pp[2 * k], pp[2 * k + 1], near, hdr[2]) ? '1' : '0');
    }
    return 0;
}
"""


def _frame_and_views(H, W):
    """A 40 x 30 frame with an offset of its own against views with different offsets (one of them none, one whose offset
    alone moves the frame's points out of its image)."""
    cam = P.offset_camera(R._camera(W, H, 0.75 * W, 0.8 * W, R._roty(2.0) @ R._rotx(-1.0), [0.03, -0.01, 0.2]), (3.3, -2.6))
    I = np.eye(3)
    views = [P.offset_camera(R._moved(cam, I, [0, 0, 0]), (3.3, -2.6)),           # its own camera
             R._moved(cam, I, [0, 0, 0]),                                         # the same pose, no offset
             P.offset_camera(R._moved(cam, I, [0, 0, 0]), (-7.75, 5.5)),
             P.offset_camera(R._moved(cam, I, [0, 0, 0]), (3.3 + 2.0 * W, -2.6)),  # the offset alone: out of the image
             P.offset_camera(R._moved(cam, R._roty(9.0), [0.2, 0.0, 0.1], W=W + 11, H=H + 6, fx=0.6 * W, fy=0.9 * W), (1.25, 4.0)),
             P.offset_camera(R._moved(cam, R._rotx(4.0), [0.0, 0.1, -0.8]), (-0.5, -0.5))]
    return cam, views


@pytest.mark.parametrize("stride", [1, 3])
def test_point_header_compiled_for_the_host_decides_like_the_restatement(tmp_path, stride):
    """csrc/overlap_point.h (the *_pp functions) compiled for the host: the world point of every lattice pixel equals the
    float32 restatement of the seeding ray bit for bit, and every (pixel, view) decision equals the restatement's."""
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    from gs_seed import seed_camera_pp

    src, exe = tmp_path / "main.cpp", tmp_path / "overlap_pp_host"
    src.write_text(_MAIN)
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    H, W, near = 30, 40, 0.3
    cam, views = _frame_and_views(H, W)
    z = R.range_map(H, W, seed=H + W + stride)
    ys, xs = R.lattice(H, W, stride)
    for border in (0, 2):
        blob = struct.pack("<iiif", len(views), len(ys), border, near) + bytes(seed_camera_pp(cam))
        blob += R.table_rows(views).tobytes()
        blob += np.array([principal_point_offset(v) for v in views], np.float32).tobytes()
        pts = np.zeros(len(ys), np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<f4")]))
        pts["x"], pts["y"], pts["z"] = xs, ys, z[ys, xs]
        out = subprocess.run([str(exe)], input=blob + pts.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        rec = np.frombuffer(out, np.dtype([("p", "<f4", 3), ("seen", "S%d" % len(views))]))
        assert len(rec) == len(ys)
        mys, mxs, p = P.overlap_points_f32(z, cam, stride)
        measured = np.zeros((H, W), bool)
        measured[mys, mxs] = True
        sel = measured[ys, xs]
        assert np.array_equal(rec["p"][sel].view(np.uint32), np.stack(p, 1).astype(np.float32).view(np.uint32))
        got = np.array([[ch == ord("1") for ch in s] for s in rec["seen"]])
        want = np.zeros((H, W, len(views)), bool)
        want[mys, mxs] = P.overlap_seen_f32(z, cam, views, stride, near, border).T
        assert np.array_equal(got, want[ys, xs])
        c = P.overlap_counts_f32(z, cam, views, stride, near, border)
        n_meas = int(sel.sum())
        inside = (mxs >= border) & (mxs < W - border) & (mys >= border) & (mys < H - border)
        assert c[0] == int(inside.sum())     # its own camera and offset: every point falls back on its own pixel centre
        assert 0 < c[1] < c[0] or border     # the same pose without the offset: shifted by (3.3, -2.6) pixels, some fall outside
        assert c[3] == 0 and c[len(views)] == n_meas  # the offset alone moves every point out of the image
        assert got.any() and not got.all()
    # without offsets the *_pp restatement is the centred one
    plain = R._camera(W, H, 0.75 * W, 0.8 * W, R._roty(2.0) @ R._rotx(-1.0), [0.03, -0.01, 0.2])
    pviews = [R._moved(plain, R._roty(5.0), [0.1, 0.0, 0.0]), R._moved(plain, np.eye(3), [0, 0, 0])]
    assert np.array_equal(P.overlap_seen_f32(z, plain, pviews, stride, near, 1), R.seen_f32(z, plain, pviews, stride, near, 1))


# ----------------------------------------------------------------------------------------------- 4. the z-depth conversion
@pytest.mark.parametrize("w,h,off", [(120, 90, (7.3, -4.6)), (121, 91, (21.25, -18.5)), (120, 90, (-70.5, 3.0)),
                                     (128, 96, (0.0, 0.0))])
def test_z_to_range_uses_the_rays_of_the_principal_point(w, h, off):
    """range = z sqrt(u^2 + v^2 + 1), u = (x + 0.5 - cx) / fx, v = (y + 0.5 - cy) / fy in float64, to float32 rounding: the
    conversion's rays come from float32 ray vectors (a few 2^-24 relative) and its result is rounded once more."""
    import torch

    from gs_train import z_to_range

    cam = P.offset_camera(make_camera(w, h, yaw_deg=11.0), off)
    cam.focal_y = 0.8 * w
    cam.tran = np.array([0.3, -0.2, 0.5], np.float32)
    z = np.random.default_rng(5).uniform(0.5, 9.0, (h, w)).astype(np.float32)
    got = z_to_range(torch.from_numpy(z), cam).numpy()
    cx0, cy0 = principal_point_default(w, h)
    cx, cy = cx0 + off[0], cy0 + off[1]
    u = (np.arange(w)[None, :] + 0.5 - cx) / float(cam.focal_x)
    v = (np.arange(h)[:, None] + 0.5 - cy) / float(cam.focal_y)
    want = z.astype(np.float64) * np.sqrt(u * u + v * v + 1.0)
    assert got.dtype == np.float32 and np.abs(got / want - 1.0).max() <= 8 * 2.0 ** -24
    if off != (0.0, 0.0):  # the centred rays would be off by far more than that
        centred = copy.copy(cam)
        centred.cx = centred.cy = None
        plain = z_to_range(torch.from_numpy(z), centred).numpy()
        assert np.abs(plain / want - 1.0).max() > 1e-3


# ------------------------------------------------------------------------------------------------- 5. the variants' resources
def test_the_principal_point_kernels_fit_the_budgets_of_their_twins():
    """The *_pp project kernels are compile-time variants of the kernels tests/test_kernel_resources.py pins (1,024 threads per
    workgroup: 128 VGPRs is the hard limit; no scratch), two additions longer; the seeding and overlap variants keep their
    twins' resources as well.  Read from the gfx950 code objects of the built library."""
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    kernels = {}
    for elf in code_objects(open(LIB, "rb").read()):
        kernels.update(kernel_metadata(elf))

    def pick(part):
        hits = [v for k, v in kernels.items() if part in k]
        assert len(hits) == 1, (part, [h[".name"] for h in hits])
        return hits[0]

    for pp, twin in (("frame_project_count_pp_kernelILb0E", "frame_project_count_kernelILb0E"),
                     ("frame_project_count_pp_kernelILb1E", "frame_project_count_kernelILb1E"),
                     ("frame_packed_project_count_pp_kernelILb0E", "frame_packed_project_count_kernelILb0E"),
                     ("frame_project_cull_count_pp_kernel", "frame_project_cull_count_kernel"),
                     ("frame_packed_project_cull_count_pp_kernel", "frame_packed_project_cull_count_kernel"),
                     ("frame_project_bin_count_pp_kernelILb0E", "frame_project_bin_count_kernelILb0E"),
                     ("frame_project_pp_kernel", "frame_project_kernel"),
                     ("seed_apply_pp_kernelILi3E", "seed_apply_kernelILi3E"),
                     ("overlap_count_pp_kernel", "overlap_count_kernel")):
        a, b = pick(pp), pick(twin)
        assert a[".vgpr_count"] <= 128 and a[".vgpr_count"] <= b[".vgpr_count"] + 4, (pp, a[".vgpr_count"], b[".vgpr_count"])
        assert a[".vgpr_spill_count"] == 0 and a[".private_segment_fixed_size"] == 0, pp
        assert a[".group_segment_fixed_size"] == b[".group_segment_fixed_size"], pp
        assert a[".max_flat_workgroup_size"] == b[".max_flat_workgroup_size"], pp
