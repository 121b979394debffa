"""gs_testutil.general_camera has the properties that make it worth a test, and every frame stated for comparing the HIP
frame path with the oracle under it (gs_testutil.GENERAL_CASES) is a valid input -- proven here on the oracle alone, so that
a GPU comparison asserts kernels and never discovers on the device that a scene has drifted out of view."""
import numpy as np
import pytest

from gs_testutil import GENERAL_CASES, general_camera, general_frame, robust_aux_grads

SMALL_CAP = 0.005  # masked pixels as a share of the image: tests/test_gpu_aux_backward.py's cap for small frames


def test_general_camera_properties():
    cam = general_camera(128, 96)
    rot = cam.rot.astype(np.float64)
    assert cam.rot.dtype == np.float32 and cam.tran.dtype == np.float32
    mags = np.sort(np.abs(rot).ravel())
    # the default angles, measured: smallest entry 0.0248, smallest gap between two magnitudes 0.0258
    assert 0.0247 < mags[0] < 0.0249 and 0.0257 < np.diff(mags).min() < 0.0259, (mags[0], np.diff(mags).min())
    assert np.abs(rot.T @ rot - np.eye(3)).max() <= 1e-6 and np.linalg.det(rot) > 0
    assert cam.focal_x == 96.0 and cam.focal_y == float(np.float32(0.85 * 96.0))
    assert abs(cam.focal_x - cam.focal_y) >= 0.1 * cam.focal_x
    # rot = Rz(roll) Rx(pitch) Ry(yaw) in that order: rot[2] = (-cos p sin y, sin p, cos p cos y) does not see the roll
    p, y = np.radians(-12.0), np.radians(10.0)
    assert np.allclose(rot[2], [-np.cos(p) * np.sin(y), np.sin(p), np.cos(p) * np.cos(y)], atol=1e-7)
    assert np.allclose(np.arctan2(rot[1, 1], -rot[0, 1]), np.radians(90.0 - 35.0), atol=1e-6)
    # what this camera is not -- a rotation about one axis (exact zeros), fx close to fy -- is refused
    for kw in (dict(roll=30.0, pitch=0.0, yaw=0.0), dict(roll=0.0, pitch=30.0, yaw=0.0), dict(roll=0.0, pitch=0.0, yaw=30.0)):
        with pytest.raises(AssertionError):
            general_camera(128, 96, **kw)
    with pytest.raises(AssertionError):
        general_camera(128, 96, fy_ratio=0.95)
    # the tile grid sees the two focal lengths
    from gs_testutil import frame_scalars

    grid, hw, hh, rays = frame_scalars(cam)
    assert grid.tile_geo_length_x != grid.tile_geo_length_y
    assert abs(grid.tile_geo_length_y / grid.tile_geo_length_x - cam.focal_x / cam.focal_y) < 1e-5


@pytest.mark.parametrize("key", sorted(GENERAL_CASES))
def test_general_camera_case_is_a_valid_input(key):
    c = GENERAL_CASES[key]
    scene, cam, of = general_frame(key)
    lens = np.diff(of.accum)
    visible = float(of.mask.mean())
    line = f"general camera case {key}: visible {visible:.2f}, pairs {len(of.ids)}, longest list {int(lens.max())}"
    assert visible >= 0.3, line
    assert len(of.ids) > 0, line
    if c["deep"]:
        assert lens.max() > 64, line
    if c["grads"]:
        _, _, _, n_masked = robust_aux_grads(of, 1)
        line += f", masked pixels {n_masked} of {c['W'] * c['H']}"
        assert n_masked < SMALL_CAP * c["W"] * c["H"], line
    print(line)


def test_generator_figures_at_the_default_angles():
    """The figures the cases were chosen on (default angles, seed 7), so that a change of the generator or of the helper
    that moves them is seen: visible share to two places; pair count, longest list and masked pixels exactly."""
    scene, cam, of = general_frame("pose")
    assert (round(float(of.mask.mean()), 2), len(of.ids), int(np.diff(of.accum).max())) == (0.72, 12_147, 395)
    for key, vis, masked in (("pose", 0.72, 26), ("fwd_256", 0.73, 11), ("fwd_333", 0.70, 80), ("fwd_40", 0.36, 6),
                             ("aux_sh2", 0.71, 19)):
        assert abs(float(general_frame(key)[2].mask.mean()) - vis) < 0.01, key
        assert robust_aux_grads(general_frame(key)[2], 1)[3] == masked, key
    assert int(np.diff(general_frame("fwd_333")[2].accum).max()) == 479
    assert int(np.diff(general_frame("aux_sh2")[2].accum).max()) == 342
