"""GPU parity under a GENERAL camera (gs_testutil.general_camera: rot = Rz(35) Rx(-12) Ry(10), fy = 0.85 fx).

Every other comparison of a HIP kernel with the oracle uses gs_scene.make_camera: a rotation about +y -- four entries of rot
exactly 0, one exactly 1 -- and fx = fy, under which a kernel that reads rot[1] for rot[3], drops a y-row term or takes focal_x
for focal_y renders the same frame.  This file runs the bodies of those tests -- the reference API (test_gpu_kernels.py), the
fused frame forward and backward (test_gpu_frame.py), the depth / alpha maps (test_gpu_aux.py, test_gpu_aux_backward.py), the
fused Adam step (test_gpu_rgbd.py), the pose gradient (test_gpu_pose.py) and the occlusion cull's random walk -- with their
tolerances unchanged on the frames of gs_testutil.GENERAL_CASES, each of which tests/test_general_camera_host.py proves a valid
input on the CPU.  An oracle frame is computed once per case (gs_testutil.general_frame) and shared, read only.

Each comparison prints a line "GENCAM ..." with the worst err / tol the helpers return: profiles/general_camera_parity.txt.
"""
import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import Camera
from gs_testutil import (GENERAL_CASES, assert_grads_close, general_camera, general_case, general_frame, general_rotation,
                         robust_aux_grads, to_torch)
from test_gpu_aux import check_maps
from test_gpu_aux_backward import SMALL_CAP, _backward_three_ways, _forward
from test_gpu_frame import IMG_ATOL, _dense_case, check_forward
from test_gpu_kernels import (check_calc_tile_list_and_gather, check_draw_forward_backward, check_global_culling_backward,
                              check_global_culling_forward, check_world2camera_and_jacobian)
from test_gpu_pose import _identity_case, check_pose_gradient
from test_gpu_rgbd import _assert_same, _fused_pair

pytestmark = pytest.mark.gpu

COLOUR_KEYS = ["rgb", "sh2", "sh3"]


def _worst(report):
    """assert_grads_close's / assert_rows_close's report -> {name: worst err / tol}"""
    return {k: v[0] for k, v in report.items()}


def _forward_parity(gpu, key, what, **kw):
    """check_forward on GENERAL_CASES[key]: pair list, tile ranges and projected records bit for bit, image within IMG_ATOL."""
    scene, cam, of = general_frame(key)
    of, r, params = check_forward(gpu, scene, cam, of=of, **kw)
    image, _ = r.forward(*params, cam)
    print(f"GENCAM forward {key} {what}: pairs {len(of.ids)}, lists bit-exact, image err/tol",
          round(float(np.abs(image.cpu().numpy() - of.image).max()) / IMG_ATOL, 3))
    return of, r, params


def _image_backward(gpu, key, what, r_kw=None, img_atol=IMG_ATOL, seed=4, **tol):
    """render + backward of GENERAL_CASES[key] on white-noise dL/dimage (zero where the stop decision is not robust) against
    OracleFrame.backward, element by element.  -> (oracle frame, renderer, gradients, reference, scale)"""
    scene, cam, of = general_frame(key)
    gimg = np.random.default_rng(seed).normal(size=of.image.shape).astype(np.float32)
    gimg, n_masked = of.robust_grad_image(gimg)
    assert n_masked < SMALL_CAP * gimg.shape[0] * gimg.shape[1], n_masked
    ref, scale = of.backward(gimg, with_scale=True)
    params = to_torch(scene, gpu, requires_grad=True)
    grow = "tile_culling_method" in (r_kw or {})  # "dist" frames: the rows cover the bounding squares
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + (0 if grow else 5), training=True, auto_grow=grow, **(r_kw or {}))
    if grow:
        r.forward(*params, cam)
        r.auto_grow = False
    img = r.render(*params, cam)
    st = r.stats()
    assert st.overflow == 0 and st.pairs == len(of.ids) and st.visible == int(of.mask.sum())
    v = r.debug_views()
    assert np.array_equal(v["sorted_keys"].cpu().numpy().view(np.uint64), of.keys), "sorted (tile, depth) keys differ"
    assert np.array_equal(v["sorted_ids"].cpu().numpy(), of.ids), "sorted Gaussian ids differ from the oracle"
    assert np.abs(img.detach().cpu().numpy() - of.image).max() < img_atol
    img.backward(torch.from_numpy(gimg).to(gpu))
    grads = [t.grad.cpu().numpy() for t in params]
    report = assert_grads_close(grads, ref, scale, f"general camera, {what}", **tol)
    culled = of.mask == 0
    for g in grads:
        assert np.abs(g[culled]).max(initial=0.0) == 0.0, what  # culled Gaussians get exactly zero
    print(f"GENCAM backward {key} {what}: masked pixels {n_masked}, worst err/tol", _worst(report))
    return of, r, grads, ref, scale


# ------------------------------------------------------------------------------------------------------- reference API
def test_global_culling_forward_bit_exact(gpu):
    scene, cam, _ = general_case("api_cull")
    check_global_culling_forward(gpu, scene, cam)
    print("GENCAM global_culling forward api_cull: mask equal, pos_i and cov bit for bit")


def test_global_culling_backward(gpu):
    scene, cam, _ = general_case("api_cull")
    print("GENCAM global_culling_backward api_cull: worst err/tol", check_global_culling_backward(gpu, scene, cam))


def test_world2camera_and_jacobian(gpu):
    check_world2camera_and_jacobian(gpu, general_camera(320, 200))


@pytest.mark.parametrize("method", [2, 1, 0])
def test_calc_tile_list_and_gather(gpu, method):
    """tile_geo_length_y != tile_geo_length_x: the three listing methods' y extents."""
    scene, cam, _ = general_case("api_tiles")
    check_calc_tile_list_and_gather(gpu, scene, cam, method)


@pytest.mark.parametrize("colour", ["rgb", "sh2"])
def test_draw_forward_backward(gpu, colour):
    _, _, of = general_frame("api_draw_" + colour)
    report = check_draw_forward_backward(gpu, of, colour != "rgb")
    print(f"GENCAM draw_backward rows api_draw_{colour}: worst err/tol", _worst(report))


# -------------------------------------------------------------------------------------------------- fused frame forward
@pytest.mark.parametrize("sort_mode", [2, "2t"])
@pytest.mark.parametrize("key", ["fwd_256", "fwd_333", "fwd_40"])
def test_frame_forward_parity(gpu, key, sort_mode):
    _forward_parity(gpu, key, f"sort_mode {sort_mode}", sort_mode=sort_mode)


@pytest.mark.parametrize("sort_mode", [0, 1, "2s"])
def test_frame_forward_parity_fallback_variants(gpu, sort_mode):
    _forward_parity(gpu, "fwd_333", f"sort_mode {sort_mode}", sort_mode=sort_mode)


@pytest.mark.parametrize("key", ["fwd_prob", "fwd_dist_0.5", "fwd_dist_0.3"])
def test_frame_tile_culling_methods(gpu, key):
    """"prob": the bounding box against the tiles' edges; "dist": the disc of tiles whose centres are near, walked over its
    bounding square -- both with a y extent in tile_geo_length_y: the pair list equals the oracle's calc_tile_list bit for
    bit, image and gradients follow."""
    c = GENERAL_CASES[key]
    _image_backward(gpu, key, c["method"], seed=6,
                    r_kw=dict(tile_culling_method=c["method"], tile_culling_dist_thresh=c["dist"]))


@pytest.mark.parametrize("degree", [2, 3])
def test_frame_forward_sh(gpu, degree):
    """The ray basis built on the device against RayBasis (pinned to the reference by tests/golden/host_geometry.npz)."""
    _forward_parity(gpu, f"fwd_sh{degree}", f"SH degree {degree}")


@pytest.mark.parametrize("sort_mode", [2, "2t"])
def test_frame_forward_emitted_sorted_keys(gpu, sort_mode):
    _forward_parity(gpu, "fwd_256", f"emitted keys, sort_mode {sort_mode}", sort_mode=sort_mode, emit_sorted_keys=True)


# --------------------------------------------------------------------------------------------------- depth / alpha maps
@pytest.mark.parametrize("colour", COLOUR_KEYS)
@pytest.mark.parametrize("training", [False, True])
def test_aux_forward_parity(gpu, colour, training):
    scene, cam, of = general_frame("aux_" + colour)
    r = FrameRenderer(gpu, max_pairs=len(of.ids) + 64, training=training, auto_grow=False)
    image, padded, depth, alpha = r.forward(*to_torch(scene, gpu), cam, aux=True)
    assert r._frame.flags & _lib.GS_FRAME_AUX
    assert r.stats().pairs == len(of.ids)
    assert np.abs(image.cpu().numpy() - of.image).max() < IMG_ATOL
    ref = check_maps(of, depth, alpha, r._aux_keep[2] if training else None)
    g = of.grid
    dscale = max(1.0, float(np.abs(of.s_pos[:, 2]).max()))
    print(f"GENCAM aux forward aux_{colour} training={training}: err/tol image",
          round(float(np.abs(image.cpu().numpy() - of.image).max()) / IMG_ATOL, 3), "alpha",
          round(float(np.abs(alpha.cpu().numpy() - g.crop(ref[:, :, 1:2])[:, :, 0]).max()) / IMG_ATOL, 3), "depth",
          round(float(np.abs(depth.cpu().numpy() - g.crop(ref[:, :, 0:1])[:, :, 0]).max()) / (IMG_ATOL * dscale), 3))


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("colour", COLOUR_KEYS)
def test_frame_backward_parity(gpu, colour):
    scene, cam, of = general_frame("bwd_" + colour)
    check_forward(gpu, scene, cam, training=True, of=of)
    _image_backward(gpu, "bwd_" + colour, colour)


def test_rgb_backward_row_layout_matches_oracle(gpu):
    """raster_backward_rows_kernel (GS_FRAME_BWD_ROWS) in both binning variants, and against the pixel-parallel kernel."""
    got = {}
    for strips in (True, False):
        _, r, got[strips], _, _ = _image_backward(gpu, "bwd_rgb", f"row layout, strips={strips}", seed=8,
                                                  r_kw=dict(bwd_rows=True, force_strips=strips))
        assert r._frame.flags & 64 and r.binning_variant() == ("strip" if strips else "table")
    _, r, plain, _, _ = _image_backward(gpu, "bwd_rgb", "pixel-parallel", seed=8, r_kw=dict(bwd_rows=False))
    assert not (r._frame.flags & 64)
    for a, b, t in zip(got[True], plain, ("pos", "quat", "scale", "opa", "rgb")):
        assert np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b.astype(np.float64)) + 1e-300) < 2e-5, t


def test_frame_backward_workgroup_summed_gaussians(gpu):
    """max_px_sigma = 48: Gaussians of more than 64 tiles, whose rows the projection backward sums by the whole workgroup."""
    of, r, grads, ref, scale = _image_backward(gpu, "bwd_wide", "workgroup-summed", seed=7)
    rc = r._rects().cpu().numpy()
    big = np.nonzero((rc[:, 2] != 0) & (rc[:, 3] > 64) & (of.mask != 0))[0]
    assert len(big) > 0
    report = assert_grads_close([g[big] for g in grads], {k: v[big] for k, v in ref.items()},
                                {k: v[big] for k, v in scale.items()}, "general camera, the workgroup-summed ones", l2=1e-4)
    print(f"GENCAM backward bwd_wide the {len(big)} Gaussians of more than 64 tiles: worst err/tol", _worst(report))


def test_frame_backward_exp_scale_activation(gpu):
    """Tolerances: test_gpu_frame.py::test_frame_backward_exp_scale_activation's (expf differs by ulps before projection)."""
    _image_backward(gpu, "bwd_exp", "exp scales", seed=5, r_kw=dict(scale_activation="exp"), img_atol=2e-4,
                    rtol=1e-3, kappa=1e-4, l2=1e-3)


def test_frame_tile_culling_method_dist_sh_backward(gpu):
    c = GENERAL_CASES["bwd_dist_sh2"]
    _image_backward(gpu, "bwd_dist_sh2", "dist, SH", seed=6,
                    r_kw=dict(tile_culling_method="dist", tile_culling_dist_thresh=c["dist"]))


@pytest.mark.parametrize("colour", ["rgb", "sh2"])
def test_aux_backward_three_ways(gpu, colour):
    """test_gpu_aux_backward.py::test_translucent's "base" scene: all three gradients, the maps alone, the depth map alone."""
    key = "aux3_" + colour
    scene, cam, of = general_frame(key)
    assert np.diff(of.accum).max() > 64
    gimg, gd, ga, n_masked = robust_aux_grads(of, 101)
    assert n_masked < SMALL_CAP * cam.width * cam.height, n_masked
    r, _, _ = _forward(gpu, of, scene, cam, {})
    reports = _backward_three_ways(gpu, r, of, scene, gimg, gd, ga, f"general camera {key}")
    for way, (got, ref, scale) in reports.items():
        print(f"GENCAM aux backward {key} [{way}]: masked pixels {n_masked}, worst err/tol",
              _worst(assert_grads_close(got, ref, scale, f"{key} [{way}]")))


@pytest.mark.parametrize("aux", [False, True])
def test_fused_backward_adam_equals_backward_then_adam(gpu, aux):
    """gs_frame_backward_adam / gs_frame_backward_adam_aux: parameters, both moments and the gradient statistic bit for bit."""
    scene, cam, _ = general_case("adam")
    _assert_same(_fused_pair(gpu, scene, cam, "max", True, 4, max_pairs=1 << 20, aux=aux), "max")
    print(f"GENCAM fused backward + Adam adam aux={aux}: bit-equal to backward then Adam over 4 steps")


# -------------------------------------------------------------------------------------------------------- pose gradient
@pytest.mark.parametrize("aux", [False, True])
def test_pose_gradient_matches_fp64_oracle(gpu, aux):
    scene, cam, of = general_frame("pose")
    print(f"GENCAM pose gradient pose aux={aux}: worst err/tol", round(check_pose_gradient(gpu, scene, cam, aux, of=of), 3))


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("bwd_rows", [False, True])
def test_pose_identities(gpu, aux, bwd_rows):
    scene, cam, _ = general_case("pose_identity")
    _identity_case(gpu, scene, cam, aux, bwd_rows, 43)


# --------------------------------------------------------------------------------------- occlusion cull, 6-DoF motion
def test_occlusion_cull_six_dof_walk_is_bit_exact(gpu):
    """test_gpu_frame.py::test_occlusion_cull_random_walk_is_bit_exact's loop from general_camera's pose, fx != fy throughout:
    120 frames, each of which rests (a quarter), steps ONE of roll, pitch and yaw by 0.001 ... 3 degrees (log-uniform, either
    sign) or one of the translation's x, y, z by N(0, 0.003) -- against a renderer with the cull off, bit for bit.  How often the
    renderer's policy culls is not a property of the kernels: at least one frame culled and one with dilated cuts is asserted.
    Measured on an MI355X with this seed: 78 of the 120 frames culled, 59 of them with dilated cuts
    (profiles/general_camera_parity.txt)."""
    W, H = 320, 208
    scene, _ = _dense_case(n=150_000, W=W, H=H, seed=17)
    start = general_camera(W, H)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False)
    off = FrameRenderer(gpu, max_pairs=1 << 22, auto_grow=False, occlusion_cull=False)
    rng = np.random.default_rng(3)
    angles0 = np.array([35.0, -12.0, 10.0])
    angles, tran = angles0.copy(), np.asarray(start.tran, np.float64).copy()
    culled = dilated = 0
    for k in range(120):
        u = rng.random()
        if 0.25 <= u < 0.9:
            a = int(rng.integers(3))
            step = np.exp(rng.uniform(np.log(0.001), np.log(3.0))) * (1 if rng.random() < 0.5 else -1)
            angles[a] = float(np.clip(angles[a] + step, angles0[a] - 20, angles0[a] + 20))
        elif u >= 0.9:
            tran[int(rng.integers(3))] += float(rng.normal(0.0, 0.003))
        cam = Camera(W, H, start.focal_x, start.focal_y, general_rotation(*angles), tran.astype(np.float32))
        img, _ = r.forward(*params, cam)
        assert r.stats().overflow == 0
        ref, _ = off.forward(*params, cam)
        assert torch.equal(img, ref), (k, angles, tran, int(r._frame.flags), r.stats())
        culled += int(bool(r._frame.flags & 256))
        dilated += int(bool(r._frame.flags & 512))
    print(f"GENCAM occlusion cull, 6-DoF walk of 120 frames: culled {culled}, of which with dilated cuts {dilated}")
    assert culled >= 1 and dilated >= 1, (culled, dilated)
