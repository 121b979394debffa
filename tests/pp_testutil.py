"""Shared helpers of the principal-point tests (GS_FRAME_PRINCIPAL_POINT, include/gs_abi.h; gs_scene.Camera.cx / cy).

The yardstick is the oracle's own staged pipeline with ONE step restated: ``PPOracleFrame`` runs oracle.global_culling with half
extents that cull nothing, adds (sx, sy) to the first two columns in float32, re-derives the mask from ``near`` and the SHIFTED
centre against the real half extents, and hands that to oracle.sorted_pairs / calc_tile_list, oracle.draw and the backward chain
as they are, with the ray basis of the moved principal point.  Nothing under oracle/ is touched.

The float32 restatements of the seeding ray and of the overlap decision for offset cameras are here as well (the centred ones:
tests/seed_ref.py, tests/overlap_ref.py)."""
import copy

import numpy as np

import oracle
from gs_geometry import RayBasis, TileGrid, principal_point_default, principal_point_offset
from gs_testutil import OracleFrame, activate, sigmoid32
from overlap_ref import _cam_arrays, _counts, measured_lattice, origin

F = np.float32

# offsets in pixels, added to (cx0, cy0): fractional; more than a tile (tile indices move); the principal point outside a
# 120-pixel-wide image, as in a crop of a larger sensor
OFFSETS = ((7.3, -4.6), (21.25, -18.5), (-70.5, 3.0))
SIZES = ((128, 96), (120, 90), (121, 91))  # no padding; padded on both axes; odd (the 0.5 of cx0)


def offset_camera(cam, off):
    """A copy of ``cam`` whose principal point lies ``off`` = (dx, dy) pixels from the renderer's centre."""
    c = copy.copy(cam)
    cx0, cy0 = principal_point_default(cam.width, cam.height)
    c.cx, c.cy = cx0 + off[0], cy0 + off[1]
    return c


def centre_shift(cam):
    """(sx, sy) as the library forms them: the offset in double over the frame's float32 focal length, rounded once."""
    dx, dy = principal_point_offset(cam)
    return F(dx / float(F(cam.focal_x))), F(dy / float(F(cam.focal_y)))


def shifted_projection(scene, cam, qn=None, sn=None, scale_activation="abs"):
    """(pos_i [N,3], cov [N,2,2], mask [N] int64) of the frame's projection with the shifted centre: oracle.global_culling with
    half extents that cull nothing (its mask is then the near-plane test alone), (sx, sy) added to the first two columns in
    float32, the mask re-derived from ``near`` and the SHIFTED centre against the real half extents."""
    if qn is None:
        qn, sn = activate(scene, scale_activation)
    grid = TileGrid(cam.width, cam.height, cam.focal_x, cam.focal_y)
    hw, hh = grid.frustum_half_extents()
    big = 1.0e30
    pos_i, cov, near_mask = oracle.global_culling(scene.pos, qn, sn, cam.rot, cam.tran, cam.near, big, big)
    sx, sy = centre_shift(cam)
    pos_i[:, 0] = pos_i[:, 0] + sx  # float32, one rounding
    pos_i[:, 1] = pos_i[:, 1] + sy
    mask = (near_mask != 0) & ~((np.abs(pos_i[:, 0]) >= F(hw)) | (np.abs(pos_i[:, 1]) >= F(hh)))
    pos_i[~mask] = 0  # (the operator leaves the rows of culled Gaussians zero)
    cov[~mask] = 0
    return pos_i, cov, mask.astype(np.int64)


class PPOracleFrame(OracleFrame):
    """``OracleFrame`` for a camera with ``cx`` / ``cy``: its __init__ restated with the shifted centre (see the module text)."""

    def __init__(self, scene, cam, thresh=0.05, scale_activation="abs", tile_culling_method="prob2", dist_thresh=0.5):
        self.scene, self.cam = scene, cam
        self.dist_thresh = dist_thresh
        self.scale_activation = scale_activation
        grid = TileGrid(cam.width, cam.height, cam.focal_x, cam.focal_y)
        rays = RayBasis.from_camera(cam.rot, cam.tran, grid.padded_height, grid.padded_width, grid.focal_x, grid.focal_y,
                                    pp_offset=principal_point_offset(cam))
        self.grid, self.rays = grid, rays
        self.qn, self.sn = activate(scene, scale_activation)
        self.pos_i, self.cov, self.mask = shifted_projection(scene, cam, self.qn, self.sn)
        if tile_culling_method == "prob2":
            self.keys, self.ids, self.accum = oracle.sorted_pairs(
                self.pos_i, self.cov.reshape(-1, 4), self.mask, thresh, grid.tile_geo_length_x,
                grid.tile_geo_length_y, grid.n_tile_x, grid.n_tile_y, grid.leftmost, grid.topmost)
        else:
            self.keys, self.ids, self.accum = self._pairs_from_table(tile_culling_method, thresh)
        self.opa_act = sigmoid32(scene.opa)
        self.col_act = scene.rgb if scene.use_sh else sigmoid32(scene.rgb)
        ids = self.ids
        self.s_pos, self.s_cov = self.pos_i[ids], self.cov.reshape(-1, 4)[ids]
        self.s_opa, self.s_rgb = self.opa_act[ids], self.col_act[ids]
        self.padded = oracle.draw(self.s_pos, self.s_rgb, self.s_opa, self.s_cov, self.accum, grid.padded_height,
                                  grid.padded_width, grid.focal_x, grid.focal_y, use_sh=scene.use_sh, fast=True,
                                  rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx, vdy=rays.dy)
        self.image = grid.crop(np.clip(self.padded, 0, 1))


# ---------------------------------------------------------------------------------------------- seeding and overlap in float32
def seed_ray_f32(cam, ys, xs):
    """(u, v) float32 of the seeding ray of an offset camera: u = fl(fl(fl((float)(x + x0) + 0.5f) - (float)dx) / fx)."""
    dx, dy = principal_point_offset(cam)
    fx, fy = F(cam.focal_x), F(cam.focal_y)
    un = ((np.asarray(xs) + origin(cam.width)).astype(F) + F(0.5)) - F(dx)
    vn = ((np.asarray(ys) + origin(cam.height)).astype(F) + F(0.5)) - F(dy)
    return (un / fx).astype(F), (vn / fy).astype(F)


def seed_rows_f32(z, cam, ys, xs, stride, scale_factor, scale_activation="abs"):
    """(pos [n,3], raw scale [n]) float32 of the Gaussians seeded at the pixels (ys, xs) with ranges z [H,W], in seed.hip's
    operation order, one rounding per operation.  ("exp": the stored value is logf(sigma), not restated bit for bit.)"""
    rot, tran, fx, fy = _cam_arrays(cam, F)
    u, v = seed_ray_f32(cam, ys, xs)
    r = np.asarray(z, F)[ys, xs]
    zc = (r / np.sqrt(u * u + v * v + F(1.0), dtype=F)).astype(F)
    q0, q1, q2 = u * zc - tran[0], v * zc - tran[1], zc - tran[2]
    pos = np.stack([rot[k] * q0 + rot[3 + k] * q1 + rot[6 + k] * q2 for k in range(3)], 1).astype(F)
    k_sigma = F(scale_factor) * F(stride)
    f_mean = (fx + fy) * F(0.5)
    sigma = (k_sigma * zc / f_mean).astype(F)
    assert scale_activation == "abs"
    return pos, np.maximum(sigma - F(1e-4), F(0)).astype(F)


def overlap_points_f32(z, cam, stride):
    """(ys, xs, p [3][n]) of the measured lattice pixels: the world points gs_seed_apply_pp writes (overlap_point.h)."""
    ys, xs, r = measured_lattice(z, stride)
    rot, tran, _, _ = _cam_arrays(cam, F)
    u, v = seed_ray_f32(cam, ys, xs)
    zc = r / np.sqrt(u * u + v * v + F(1.0))
    q0, q1, q2 = u * zc - tran[0], v * zc - tran[1], zc - tran[2]
    return ys, xs, [rot[k] * q0 + rot[3 + k] * q1 + rot[6 + k] * q2 for k in range(3)]


def overlap_seen_f32(z, cam, views, stride, near, border):
    """bool [n_views, measured lattice pixels]: gs_overlap_seen_pp in float32, every bound moved by the view's own offset."""
    _, _, p = overlap_points_f32(z, cam, stride)
    out = np.zeros((len(views), len(p[0])), bool)
    for k, view in enumerate(views):
        rot, tran, fx, fy = _cam_arrays(view, F)
        dx, dy = (F(v) for v in principal_point_offset(view))
        qx = rot[0] * p[0] + rot[1] * p[1] + rot[2] * p[2] + tran[0]
        qy = rot[3] * p[0] + rot[4] * p[1] + rot[5] * p[2] + tran[1]
        qz = rot[6] * p[0] + rot[7] * p[1] + rot[8] * p[2] + tran[2]
        ox, oy = origin(view.width), origin(view.height)
        ax, ay = fx * qx, fy * qy
        x_lo, x_hi = F(border + ox) - dx, F(int(view.width) - border + ox) - dx
        y_lo, y_hi = F(border + oy) - dy, F(int(view.height) - border + oy) - dy
        out[k] = (qz > F(near)) & (ax >= x_lo * qz) & (ax < x_hi * qz) & (ay >= y_lo * qz) & (ay < y_hi * qz)
    return out


def overlap_counts_f32(z, cam, views, stride, near, border):
    return _counts(overlap_seen_f32(z, cam, views, stride, near, border))
