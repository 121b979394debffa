"""Shared helpers for the parity tests: oracle-side frame pipeline and comparisons."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle
from gs_geometry import RayBasis, TileGrid
from gs_scene import Camera, Scene


FAKE = 1 << 40  # a device address that is never dereferenced


def fake_frame(pose=False, aux=False, color_dim=3, training=1, N=1000, W=128, H=96):
    """A well-formed frame descriptor with fake (never dereferenced) device addresses: only host-side entry points that
    validate and return before any launch may be called with it."""
    from gaussian import _lib

    f = _lib.GsFrame()
    f.N, f.color_dim, f.scale_activation = N, color_dim, 0
    f.pos, f.quat, f.scale, f.opa, f.rgb = FAKE, FAKE + 4096, FAKE + 8192, FAKE + 12288, FAKE + 16384
    f.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    f.near_plane, f.half_width, f.half_height = 0.01, 1.0, 1.0
    f.width, f.height, f.focal_x, f.focal_y = W, H, 0.75 * W, 0.75 * W
    f.thresh, f.max_pairs, f.sort_mode, f.tile_culling_method = 0.05, 50_000, 2, 2
    f.workspace = FAKE + (1 << 30)
    f.workspace_bytes = _lib.gs_frame_workspace_bytes(f.N, f.max_pairs, W, H, color_dim, training)
    f.training = training
    f.image, f.image_padded = FAKE + (2 << 30), FAKE + (3 << 30)
    if aux:
        f.flags |= _lib.GS_FRAME_AUX
        f.aux_workspace = FAKE + (4 << 30)
        f.aux_workspace_bytes = _lib.gs_frame_aux_workspace_bytes(f.max_pairs, W, H, training)
        f.aux_padded = FAKE + (5 << 30)
    if pose:
        f.flags |= _lib.GS_FRAME_POSE_GRAD
        f.grad_rot, f.grad_tran = FAKE + (6 << 30), FAKE + (6 << 30) + 64
        f.pose_workspace = FAKE + (7 << 30)
        f.pose_workspace_bytes = _lib.gs_frame_pose_workspace_bytes(f.N)
    return f


def fake_adam(good=True):
    """A gs_adam_fused that passes gs_validate_adam_fused (fake, 16-byte aligned moments) -- or, good=False, one that does
    not (all-zero: step 0)."""
    from gaussian import _lib

    a = _lib.GsAdamFused()
    if good:
        for k in range(5):
            a.exp_avg[k] = FAKE + (8 << 30) + k * 65536
            a.exp_avg_sq[k] = FAKE + (9 << 30) + k * 65536
            a.lr[k] = 1e-3
        a.beta1, a.beta2, a.eps, a.step = 0.9, 0.99, 1e-8, 1
    return a


def sigmoid32(x):
    x = np.asarray(x, np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def activate(scene: Scene, scale_activation="abs"):
    """splatter.py:519-524 in fp32 (same expression order as the kernels)."""
    q = scene.quat.astype(np.float32)
    nr = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3], dtype=np.float32)
    qn = (q / nr[:, None]).astype(np.float32)
    if scale_activation == "abs":
        sn = (np.abs(scene.scale) + np.float32(1e-4)).astype(np.float32)
    else:
        sn = np.exp(scene.scale, dtype=np.float32)
    return qn, sn


def frame_scalars(cam: Camera):
    grid = TileGrid(cam.width, cam.height, cam.focal_x, cam.focal_y)
    hw, hh = grid.frustum_half_extents()
    rays = RayBasis.from_camera(cam.rot, cam.tran, grid.padded_height, grid.padded_width, grid.focal_x, grid.focal_y)
    return grid, hw, hh, rays


class OracleFrame:
    """Oracle restatement of one forward frame on raw parameters, keeping every intermediate."""

    def __init__(self, scene: Scene, cam: Camera, thresh=0.05, scale_activation="abs", tile_culling_method="prob2",
                 dist_thresh=0.5, activated=None):
        """``activated`` = (normalised quaternions, activated scales) computed by the CALLER (the reference's torch ops,
        splatter.py:519-524, whose last bits differ from ``activate``'s expression order): the frame is then the oracle's
        on exactly those inputs -- what the reference-API tests need to compare bit for bit behind torch activations."""
        self.scene, self.cam = scene, cam
        self.dist_thresh = dist_thresh
        self.scale_activation = scale_activation
        grid, hw, hh, rays = frame_scalars(cam)
        self.grid, self.rays = grid, rays
        self.qn, self.sn = activate(scene, scale_activation) if activated is None else \
            tuple(np.ascontiguousarray(a, np.float32) for a in activated)
        self.pos_i, self.cov, self.mask = oracle.global_culling(scene.pos, self.qn, self.sn, cam.rot, cam.tran,
                                                                cam.near, hw, hh)
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

    def robust_grad_image(self, grad_image, band=2e-5):
        """dL/dimage with the pixels zeroed whose early-stop decision is not robust in fp32 (their transmittance
        passes within its own fp32 uncertainty -- ``band`` plus what nearly opaque Gaussians in front add -- of the 1e-4
        threshold: oracle.draw_ambiguous) -- typically ~0.1 % of the pixels.
        Every gradient term is proportional to its pixel's dL/dimage, so with this input two evaluations that stop
        such a pixel one Gaussian apart still have the same set of terms to compare.  -> (grad_image, #pixels zeroed)"""
        grid = self.grid
        amb = oracle.draw_ambiguous(self.s_pos, self.s_opa, self.s_cov, self.accum, grid.padded_height,
                                    grid.padded_width, grid.focal_x, grid.focal_y, band)
        keep = ~grid.crop(amb[:, :, None])
        return np.ascontiguousarray(grad_image * keep, np.float32), int((~keep).sum())

    def _pairs_from_table(self, method, thresh):
        """'prob' / 'dist' (splatter.py:571-578): the oracle's restatement of calc_tile_list methods 1 / 0 (pinned
        bit for bit against the reference kernels) on the visible Gaussians, uncapped, then the canonical
        (tile, depth bits, Gaussian index) order."""
        grid = self.grid
        vis = np.nonzero(self.mask)[0]
        top, bottom, left, right = grid.tile_edges()
        th = (grid.tile_geo_length_x / self.dist_thresh) ** 2 if method == "dist" else thresh  # splatter.py:577
        cnt, lst = oracle.calc_tile_list(self.pos_i[vis], self.cov.reshape(-1, 4)[vis], len(vis), th,
                                         {"dist": 0, "prob": 1}[method], grid.tile_geo_length_x,
                                         grid.tile_geo_length_y, grid.n_tile_x, grid.n_tile_y, grid.leftmost,
                                         grid.topmost, top=top, bottom=bottom, left=left, right=right)
        tiles = np.repeat(np.arange(len(cnt)), cnt)
        ids = np.concatenate([vis[lst[t, :c]] for t, c in enumerate(cnt)]) if cnt.sum() else np.zeros(0, np.int64)
        dbits = self.pos_i[ids, 2].view(np.uint32).astype(np.uint64)
        keys = (tiles.astype(np.uint64) << np.uint64(32)) | dbits
        order = np.lexsort((ids, keys))
        accum = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        return keys[order], ids[order].astype(np.int32), accum

    def backward(self, grad_image, with_scale=False, scale_w=0.05):
        """dL/d(image) -> dict of dL/d(raw parameter), the chain splatter.py's autograd runs.

        ``with_scale``: also return, per gradient element, its conditioning scale -- the oracle's per-row scale
        (gs_oracle.c, draw_backward_impl) summed over the Gaussian's (tile, Gaussian) rows and pushed through the
        magnitudes of the (linear) projection / activation backward.  ``grad_close`` states tolerances in it."""
        sc, cam, grid, rays = self.scene, self.cam, self.grid, self.rays
        n = sc.n
        gpad = self._padded_grad_image(grad_image)
        out = oracle.draw_backward(self.s_pos, self.s_rgb, self.s_opa, self.s_cov, self.accum, self.padded,
                                   gpad, grid.focal_x, grid.focal_y, use_sh=sc.use_sh, fast=True,
                                   rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx, vdy=rays.dy,
                                   with_scale=with_scale, scale_w=scale_w)
        (gp, gr, go, gc), cs = out if with_scale else (out, None)
        self.pair_grads, self.pair_scales = (gp, gr, go, gc), cs  # the (tile, Gaussian) rows, for the reference-API tests
        # index backward (index_put accumulate) in double
        d_pos_i, d_cov, d_opa, d_col = (_sum_by_id(self.ids, a, n) for a in (gp, gc, go, gr))
        grads = self._chain(d_pos_i, d_cov, d_opa, d_col)
        if not with_scale:
            return grads
        s_pos_i, s_cov, s_opa, s_col = (_sum_by_id(self.ids, a, n) for a in (cs[0], cs[3], cs[2], cs[1]))
        return grads, self._chain_scale(s_pos_i, s_cov, s_opa, s_col)

    def _padded_grad_image(self, grad_image):
        """dL/d(image) laid into the padded frame, zero where the clamp to [0, 1] passes no gradient."""
        grid = self.grid
        top, left = grid.crop_offsets()
        gpad = np.zeros_like(self.padded)
        inside = ((self.padded >= 0) & (self.padded <= 1)).astype(np.float32)
        gpad[top:top + grid.height, left:left + grid.width] = grad_image
        gpad *= inside
        return gpad

    def _rows_f64(self, grad_image):
        """The (tile, Gaussian) rows (gp, gr, go, gc) of the image's backward in double (oracle.draw_backward_f64)."""
        sc, grid, rays = self.scene, self.grid, self.rays
        return oracle.draw_backward_f64(self.s_pos, self.s_rgb, self.s_opa, self.s_cov, self.accum,
                                        self._padded_grad_image(grad_image), grid.focal_x, grid.focal_y, use_sh=sc.use_sh,
                                        rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx, vdy=rays.dy)

    def backward_f64(self, grad_image):
        """The same chain as ``backward`` evaluated in DOUBLE on the fp32 inputs: K8 by oracle.draw_backward_f64
        (its own final colour, exp, sums -- only the stop decisions are the fp32 chain's), the index backward as a
        double sum, the projection backward as torch.autograd (float64) on oracle/torch_ref.project -- A.4 with the
        Jacobian detached, i.e. gaussian.cu:1371-1576 derived independently --, the activations in double.
        The yardstick of tests/test_grad_calibration.py.  -> ((gp, gr, go, gc) rows, {name: parameter gradient})."""
        rows = self._rows_f64(grad_image)
        gp, gr, go, gc = rows
        d_pos_i, d_cov, d_opa, d_col = (_sum_by_id(self.ids, a, self.scene.n) for a in (gp, gc, go, gr))
        return rows, self._chain_f64(d_pos_i, d_cov, d_opa, d_col)

    def _chain_f64(self, d_pos_i, d_cov, d_opa, d_col):
        """Per-Gaussian dL/d(pos_i, cov2d, activated opacity, activated colour) -> dL/d(raw parameter) in double: the
        projection backward as torch.autograd (float64) on oracle/torch_ref.project, the activations in double."""
        import torch

        from oracle import torch_ref

        sc, cam = self.scene, self.cam
        n = sc.n
        vis = np.nonzero(self.mask)[0]
        f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
        q = sc.quat.astype(np.float64)
        nr = np.linalg.norm(q, axis=1, keepdims=True)
        qh = q / nr
        # (the projection sees the fp32 activated values, like every fp32 evaluation: each stage's backward is taken
        # at the forward's stored fp32 intermediates)
        tp, tq, ts = (f64(a[vis]).requires_grad_(True) for a in (sc.pos, self.qn, self.sn))
        pos_i, cov = torch_ref.project(tp, tq, ts, f64(cam.rot), f64(cam.tran), detach_jacobian=True)
        obj = (pos_i * f64(d_pos_i[vis])).sum() + (cov.reshape(-1, 4) * f64(d_cov[vis])).sum()
        gpv, gqv, gsv = torch.autograd.grad(obj, (tp, tq, ts))
        g_pos, g_qn, g_sn = (np.zeros((n, k)) for k in (3, 4, 3))
        g_pos[vis], g_qn[vis], g_sn[vis] = gpv.numpy(), gqv.numpy(), gsv.numpy()
        g_q = (g_qn - qh * np.sum(qh * g_qn, axis=1, keepdims=True)) / nr
        g_s = g_sn * np.sign(sc.scale) if self.scale_activation == "abs" else g_sn * np.exp(np.clip(sc.scale, -1, 1))
        o = 1.0 / (1.0 + np.exp(-sc.opa.astype(np.float64)))
        g_o = d_opa * o * (1 - o)
        if sc.use_sh:
            g_c = d_col
        else:
            c = 1.0 / (1.0 + np.exp(-sc.rgb.astype(np.float64)))
            g_c = d_col * c * (1 - c)
        return {"pos": g_pos, "quat": g_q, "scale": g_s, "opa": g_o, "rgb": g_c}

    # ---- the depth / alpha maps of an aux frame (GS_FRAME_AUX): the oracle with the two maps posed as colours.
    # oracle.draw with the sorted colours (d_i, 1, 0), d_i = s_pos[:, 2] = |p_c| (the sort key), gives the padded (D, A);
    # oracle.draw_backward with those colours and the gradient (g_D, g_A, 0) gives their rows, whose per-Gaussian colour-0
    # sum is dL/dd_i and enters d_pos_i[:, 2] of the same projection chain as the image's gradient.
    def aux_maps(self):
        """Padded [padH, padW, 3]: (D, A, 0)."""
        g = self.grid
        return oracle.draw(self.s_pos, aux_colours(self), self.s_opa, self.s_cov, self.accum, g.padded_height,
                           g.padded_width, g.focal_x, g.focal_y, use_sh=False, fast=True)

    def _padded_grad_maps(self, gd, ga):
        """(g_D, g_A, 0) laid into the padded frame; no clamp mask: the maps are not clamped.  None = no such term."""
        g = self.grid
        top, left = g.crop_offsets()
        gpad = np.zeros((g.padded_height, g.padded_width, 3), np.float32)
        if gd is not None:
            gpad[top:top + g.height, left:left + g.width, 0] = gd
        if ga is not None:
            gpad[top:top + g.height, left:left + g.width, 1] = ga
        return gpad

    def aux_backward(self, gimg, gd, ga, with_scale=True):
        """The oracle's gradient of <gimg, image> + <gd, depth> + <ga, alpha> and (``with_scale``) its conditioning scale:
        the image chain (``backward``) plus the chain of the maps' rows -- colour-0 row sum added to d_pos_i[:, 2], the
        colour gradient of the aux part zero.  ``gimg`` / ``gd`` / ``ga`` = None: no such term.
        Keeps the aux pass's (tile, Gaussian) rows in ``aux_pair_grads`` (gp, gr, go, gc)."""
        g, sc = self.grid, self.scene
        n = sc.n
        cols = aux_colours(self)
        (gp, gr, go, gc), cs = oracle.draw_backward(self.s_pos, cols, self.s_opa, self.s_cov, self.accum, self.aux_maps(),
                                                    self._padded_grad_maps(gd, ga), g.focal_x, g.focal_y, use_sh=False,
                                                    fast=True, with_scale=True)
        self.aux_pair_grads = (gp, gr, go, gc)
        d_pos_i, d_cov, d_opa = (_sum_by_id(self.ids, a, n) for a in (gp, gc, go))
        d_pos_i[:, 2] += _sum_by_id(self.ids, gr[:, 0], n)
        s_pos_i, s_cov, s_opa = (_sum_by_id(self.ids, a, n) for a in (cs[0], cs[3], cs[2]))
        s_pos_i[:, 2] += _sum_by_id(self.ids, cs[1][:, 0], n)
        zc = np.zeros((n, sc.rgb.shape[1]))
        ref = self._chain(d_pos_i, d_cov, d_opa, zc)
        ref["rgb"][:] = 0.0
        scale = self._chain_scale(s_pos_i, s_cov, s_opa, zc)
        if gimg is not None:
            ref_i, scale_i = self.backward(gimg, with_scale=True)
            ref = {k: ref_i[k] + ref[k] for k in ref_i}
            scale = {k: scale_i[k] + scale[k] for k in scale_i}
        return (ref, scale) if with_scale else ref

    def aux_rows_f64(self, gd, ga):
        """The maps' (tile, Gaussian) rows (gp, gr, go, gc) in double; gr[:, 0] is the row's share of dL/dd_i."""
        g = self.grid
        return oracle.draw_backward_f64(self.s_pos, aux_colours(self), self.s_opa, self.s_cov, self.accum,
                                        self._padded_grad_maps(gd, ga), g.focal_x, g.focal_y, use_sh=False)

    def aux_backward_f64(self, gimg, gd, ga):
        """``aux_backward`` in double: the image's and the maps' rows of oracle.draw_backward_f64, summed per Gaussian,
        through ONE fp64 projection / activation chain (``_chain_f64``, what ``backward_f64`` uses).  -> {name: gradient}"""
        n = self.scene.n
        gp, gr, go, gc = self.aux_rows_f64(gd, ga)
        d_pos_i, d_cov, d_opa = (_sum_by_id(self.ids, a, n) for a in (gp, gc, go))
        d_pos_i[:, 2] += _sum_by_id(self.ids, gr[:, 0], n)
        d_col = np.zeros((n, self.scene.rgb.shape[1]))
        if gimg is not None:
            ip, ir, io, ic = self._rows_f64(gimg)
            d_pos_i, d_cov, d_opa = (a + _sum_by_id(self.ids, b, n) for a, b in ((d_pos_i, ip), (d_cov, ic), (d_opa, io)))
            d_col = _sum_by_id(self.ids, ir, n)
        return self._chain_f64(d_pos_i, d_cov, d_opa, d_col)

    def _chain(self, d_pos_i, d_cov, d_opa, d_col):
        sc, cam = self.scene, self.cam
        g_pos, g_qn, g_sn = oracle.global_culling_backward(sc.pos, self.qn, self.sn, cam.rot, cam.tran,
                                                           d_pos_i.astype(np.float32), d_cov.astype(np.float32),
                                                           self.mask)
        q = sc.quat.astype(np.float64)
        nr = np.linalg.norm(q, axis=1, keepdims=True)
        qh = q / nr
        g_q = (g_qn - qh * np.sum(qh * g_qn, axis=1, keepdims=True)) / nr
        if self.scale_activation == "abs":
            g_s = g_sn * np.sign(sc.scale)
        else:
            g_s = g_sn * np.exp(np.clip(sc.scale, -1, 1))
        o = self.opa_act.astype(np.float64)
        g_o = d_opa * o * (1 - o)
        if sc.use_sh:
            g_c = d_col
        else:
            c = self.col_act.astype(np.float64)
            g_c = d_col * c * (1 - c)
        return {"pos": g_pos.astype(np.float32), "quat": g_q.astype(np.float32), "scale": g_s.astype(np.float32),
                "opa": g_o.astype(np.float32), "rgb": g_c.astype(np.float32)}

    def _chain_scale(self, s_pos_i, s_cov, s_opa, s_col):
        """The scales pushed through K2 and the activations with every product taken between magnitudes and every
        difference replaced by the sum of its operands' magnitudes (oracle.global_culling_backward_scale)."""
        sc, cam = self.scene, self.cam
        S_pos, S_qn, S_sn = oracle.global_culling_backward_scale(sc.pos, self.qn, self.sn, cam.rot, cam.tran,
                                                                 s_pos_i, s_cov.reshape(-1, 4), self.mask)
        q = sc.quat.astype(np.float64)
        nr = np.linalg.norm(q, axis=1, keepdims=True)
        qh = np.abs(q / nr)
        S_q = (S_qn + qh * np.sum(qh * S_qn, axis=1, keepdims=True)) / nr
        S_s = S_sn if self.scale_activation == "abs" else S_sn * np.exp(np.clip(sc.scale, -1, 1))
        o = self.opa_act.astype(np.float64)
        S_o = s_opa * o * (1 - o)
        if sc.use_sh:
            S_c = s_col
        else:
            c = self.col_act.astype(np.float64)
            S_c = s_col * c * (1 - c)
        return {"pos": S_pos, "quat": S_q, "scale": S_s, "opa": S_o, "rgb": S_c}


def aux_colours(of):
    """The sorted colours that pose the depth / alpha maps as an image: (d_i, 1, 0), d_i = |p_c| (the sort key)."""
    d = of.s_pos[:, 2].astype(np.float32)
    return np.ascontiguousarray(np.stack([d, np.ones_like(d), np.zeros_like(d)], 1), np.float32)


def aux_case(n, W, H, seed=7, use_sh=False, sh_degree=2, yaw=2.0, **kw):
    """The aux tests' scene: make_scene seen from a camera yawed by ``yaw`` degrees and pushed off the origin."""
    from gs_scene import make_camera, make_scene

    scene = make_scene(n, W, H, seed=seed, use_sh=use_sh, sh_degree=sh_degree, **kw)
    cam = make_camera(W, H, yaw_deg=yaw)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    return scene, cam


def general_rotation(roll, pitch, yaw):
    """Rz(roll) Rx(pitch) Ry(yaw), degrees, formed in float64 and rounded once to float32."""
    import math

    a, b, c = (math.radians(v) for v in (roll, pitch, yaw))
    rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    ry = np.array([[math.cos(c), 0.0, math.sin(c)], [0.0, 1.0, 0.0], [-math.sin(c), 0.0, math.cos(c)]])
    return (rz @ rx @ ry).astype(np.float32)


def general_camera(W, H, roll=35.0, pitch=-12.0, yaw=10.0, fy_ratio=0.85, tran=(0.05, -0.04, 0.25)):
    """A camera none of whose rotation entries or focal lengths can stand in for another: rot = Rz(roll) Rx(pitch) Ry(yaw)
    (degrees; formed in float64, rounded once to float32), focal_x = 0.75 W, focal_y = float32(fy_ratio focal_x).
    make_camera's yaw-only matrix has four exact zeros and an exact one, and fx = fy: a kernel that reads rot[1] for rot[3],
    drops a y-row term or takes focal_x for focal_y computes the same frame under it.  The asserts below are conditions on
    the INPUT -- what makes this camera worth a test -- not measurements of anything under test."""
    rot = general_rotation(roll, pitch, yaw)
    fx = 0.75 * W
    fy = float(np.float32(fy_ratio * fx))
    mags = np.sort(np.abs(rot.astype(np.float64)).ravel())
    assert mags[0] >= 0.02, ("an entry of rot is (nearly) zero", rot)
    assert np.diff(mags).min() >= 0.02, ("two entries of rot have (nearly) the same magnitude", rot)
    r64 = rot.astype(np.float64)
    assert np.abs(r64.T @ r64 - np.eye(3)).max() <= 1e-6 and np.linalg.det(r64) > 0, rot
    assert abs(fx - fy) >= 0.1 * fx, (fx, fy)
    return Camera(W, H, fx, fy, rot, np.asarray(tran, np.float32))


def signed_raw_domain(scene, seed):
    """The raw scales of ``scene`` (make_scene's: all > 0) over the whole domain of the abs activation |s| + 1e-4, in place:
    every component given a random sign, 2 % of them set to exact zero (half +0.0, half -0.0 -- what the optimiser walks
    through and seeding writes), and the raw quaternions scaled to norms from 1e-3 to 1e3 (log-uniform).  The activated scales
    are make_scene's except at the zeros (1e-4); the normalised quaternions are its own up to rounding."""
    n = scene.n
    rng = np.random.default_rng(seed + 77)
    scene.scale *= rng.choice([-1.0, 1.0], size=scene.scale.shape).astype(np.float32)
    z = rng.choice(n * 3, size=n * 3 // 50, replace=False)
    flat = scene.scale.reshape(-1)
    assert np.shares_memory(flat, scene.scale)
    flat[z[::2]] = 0.0
    flat[z[1::2]] = -0.0
    scene.quat *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 1))).astype(np.float32)
    return scene


def spread_exp_domain(scene, cam, k):
    """``scene`` (make_scene's scales, any sign) and ``cam`` for the exp activation, in place: positions and the camera's
    translation times k, scales log(|s| k + 1e-4) -- the same scene seen k times larger from k times further away, its raw
    log-scales moved up by log k: with k = 8 they straddle both ends of the exp backward's clamp to [-1, 1]."""
    k = np.float32(k)
    scene.pos *= k
    cam.tran = (cam.tran * k).astype(np.float32)
    scene.scale = np.log(np.abs(scene.scale) * k + 1e-4).astype(np.float32)
    return scene, cam


RAW_CULL_SHAPE = (6_000, 256, 192, 41)  # n, W, H, seed
RAW_CULL_SPREAD = 8.0


def raw_cull_camera(domain, yaw=0.0):
    """make_camera yawed by ``yaw`` degrees, its translation (zero) scaled with the "exp" domain's scene."""
    from gs_scene import make_camera

    cam = make_camera(RAW_CULL_SHAPE[1], RAW_CULL_SHAPE[2], yaw_deg=yaw)
    if domain == "exp":
        cam.tran = (cam.tran * np.float32(RAW_CULL_SPREAD)).astype(np.float32)
    return cam


def raw_cull_case(domain):
    """The opaque, large-footprint scene of test_gpu_cull_exact.py::test_random_edits_with_large_footprints on the raw scale
    domain ``domain`` ("signed": signed_raw_domain, abs activation; "exp": spread_exp_domain by RAW_CULL_SPREAD), seen from
    raw_cull_camera.  -> (scene, camera, scale activation)"""
    from gs_scene import make_scene

    n, W, H, seed = RAW_CULL_SHAPE
    scene = make_scene(n, W, H, seed, max_px_sigma=64)
    scene.opa += np.float32(3.0)
    cam = raw_cull_camera("signed")
    if domain == "signed":
        return signed_raw_domain(scene, seed), cam, "abs"
    assert domain == "exp", domain
    spread_exp_domain(scene, cam, RAW_CULL_SPREAD)
    return scene, cam, "exp"


def aux_general_case(n, W, H, seed=7, use_sh=False, sh_degree=2, camera=None, **kw):
    """``aux_case``'s scene seen from ``general_camera`` (``camera``: keyword arguments for it)."""
    from gs_scene import make_scene

    scene = make_scene(n, W, H, seed=seed, use_sh=use_sh, sh_degree=sh_degree, **kw)
    return scene, general_camera(W, H, **(camera or {}))


# The frames for comparing the HIP frame path with the oracle under general_camera, stated once so that
# tests/test_general_camera_host.py can prove on the CPU that each is a valid input (enough of the scene in view, pairs to
# composite, multi-bucket tiles where the GPU test relies on them, few pixels masked for a non-robust stop decision).
#   n, W, H, seed; sh: 0 = rgb logits, 2 / 3 = SH degree; opa: shift of the opacity logits; exp: log scales for the exp
#   activation; sigma: make_scene's max_px_sigma; method / dist: tile culling method and its threshold;
#   deep: the comparison relies on a list beyond one 64-Gaussian bucket; grads: it runs a backward on robust_aux_grads;
#   signed: signed_raw_domain on the scene (abs activation); spread: spread_exp_domain's factor (with exp)
def _gc(n, W, H, seed=7, sh=0, opa=0.0, exp=False, sigma=16.0, method="prob2", dist=0.5, deep=False, grads=False,
        signed=False, spread=1.0):
    return dict(n=n, W=W, H=H, seed=seed, sh=sh, opa=opa, exp=exp, sigma=sigma, method=method, dist=dist, deep=deep,
                grads=grads, signed=signed, spread=spread)


GENERAL_CASES = {
    "api_cull": _gc(20_000, 320, 200),
    "api_tiles": _gc(3_000, 160, 96),
    "api_draw_rgb": _gc(12_000, 200, 120, seed=5, deep=True),
    "api_draw_sh2": _gc(12_000, 200, 120, seed=5, sh=2, deep=True),
    "fwd_256": _gc(10_000, 256, 256, deep=True),
    "fwd_333": _gc(30_000, 333, 201, deep=True),
    "fwd_40": _gc(3_000, 40, 200),
    "fwd_prob": _gc(15_000, 250, 186, seed=29, method="prob", grads=True),
    "fwd_dist_0.5": _gc(12_000, 250, 186, seed=29, method="dist", dist=0.5, grads=True),
    "fwd_dist_0.3": _gc(12_000, 333, 201, seed=29, method="dist", dist=0.3, grads=True),
    "fwd_sh2": _gc(8_000, 160, 96, sh=2),
    "fwd_sh3": _gc(8_000, 160, 96, sh=3),
    "aux_rgb": _gc(6_000, 160, 112),
    "aux_sh2": _gc(6_000, 160, 112, sh=2, deep=True, grads=True),
    "aux_sh3": _gc(6_000, 160, 112, sh=3),
    "bwd_rgb": _gc(20_000, 160, 112, seed=11, deep=True, grads=True),
    "bwd_sh2": _gc(9_000, 160, 112, seed=11, sh=2, deep=True, grads=True),
    "bwd_sh3": _gc(9_000, 160, 112, seed=11, sh=3, deep=True, grads=True),
    "bwd_wide": _gc(8_000, 192, 128, seed=47, sigma=48.0, grads=True),
    "bwd_exp": _gc(5_000, 96, 80, seed=13, exp=True, grads=True),
    "bwd_dist_sh2": _gc(6_000, 250, 186, seed=29, sh=2, opa=1.0, method="dist", dist=0.5, grads=True),
    "aux3_rgb": _gc(5_000, 128, 96, seed=13, opa=-4.0, deep=True, grads=True),
    "aux3_sh2": _gc(5_000, 128, 96, seed=13, sh=2, opa=-4.0, deep=True, grads=True),
    "adam": _gc(6_000, 160, 112, seed=11),
    "pose": _gc(5_000, 128, 96, deep=True, grads=True),
    "pose_identity": _gc(5_000, 128, 96, seed=41),
    # the raw scale domain beyond make_scene's positive slice (tests/test_raw_domain_host.py, tests/test_gpu_raw_domain.py)
    "raw_signed_rgb": _gc(5_000, 128, 96, seed=13, signed=True, deep=True, grads=True),
    "raw_signed_sh2": _gc(5_000, 128, 96, seed=13, sh=2, signed=True, deep=True, grads=True),
    "raw_exp_spread": _gc(5_000, 96, 80, seed=13, exp=True, spread=8.0, deep=True, grads=True),
    "raw_signed_adam": _gc(6_000, 160, 112, seed=11, signed=True),
    "raw_signed_pose": _gc(5_000, 128, 96, signed=True, deep=True, grads=True),
}
_GENERAL_FRAMES = {}


def general_case(key):
    """-> (scene, general_camera, keyword arguments of OracleFrame) of GENERAL_CASES[key], fresh arrays each call."""
    c = GENERAL_CASES[key]
    scene, cam = aux_general_case(c["n"], c["W"], c["H"], seed=c["seed"], use_sh=bool(c["sh"]), sh_degree=c["sh"] or 2,
                                  max_px_sigma=c["sigma"])
    if c["opa"]:
        scene.opa += np.float32(c["opa"])
    of_kw = {}
    if c["signed"]:
        signed_raw_domain(scene, c["seed"])
    if c["exp"] and c["spread"] != 1.0:
        spread_exp_domain(scene, cam, c["spread"])
        of_kw["scale_activation"] = "exp"
    elif c["exp"]:
        scene.scale = np.log(np.abs(scene.scale) + 1e-4).astype(np.float32)
        of_kw["scale_activation"] = "exp"
    if c["method"] != "prob2":
        of_kw.update(tile_culling_method=c["method"], dist_thresh=c["dist"])
    return scene, cam, of_kw


def general_frame(key):
    """-> (scene, camera, OracleFrame) of GENERAL_CASES[key], computed once per process and shared: read only."""
    if key not in _GENERAL_FRAMES:
        scene, cam, of_kw = general_case(key)
        _GENERAL_FRAMES[key] = (scene, cam, OracleFrame(scene, cam, **of_kw))
    return _GENERAL_FRAMES[key]


def robust_aux_grads(of, rng, image=True):
    """White-noise dL/dimage [H,W,3] (zeros if not ``image``), dL/ddepth, dL/dalpha [H,W] from ``rng`` (a seed or a numpy
    Generator), all three zeroed on the pixels whose early-stop decision is not robust in fp32
    (OracleFrame.robust_grad_image).  -> (gimg, gd, ga, number of pixels masked): the caller caps that number."""
    g = of.grid
    rng = np.random.default_rng(rng)
    gimg = rng.normal(size=of.image.shape).astype(np.float32) if image else np.zeros(of.image.shape, np.float32)
    gimg_r, n_masked = of.robust_grad_image(np.ones(of.image.shape, np.float32))
    keep = gimg_r[:, :, 0]  # 1 where the pixel's stop decision is robust, 0 where it is ambiguous
    gimg = gimg * keep[:, :, None]
    gd = (rng.normal(size=(g.height, g.width)) * keep).astype(np.float32)
    ga = (rng.normal(size=(g.height, g.width)) * keep).astype(np.float32)
    return gimg, gd, ga, n_masked


def saturated_share(of, aux_padded=None):
    """Share of the image's pixels that stopped inside their list: oracle alpha > 0.9999 (transmittance below the 1e-4
    stop threshold)."""
    a = of.grid.crop((of.aux_maps() if aux_padded is None else aux_padded)[:, :, 1:2])[:, :, 0]
    return float(np.mean(a > 0.9999))


def depth_loss_f64(D, A, z, mode, alpha_min, scale):
    """gs_loss_depth's formulas in float64 (the reference of tests/test_gpu_rgbd.py::test_depth_loss_matches_fp64):
    scale x sum |r| over the measured pixels (z finite and > 0; "expected": and A >= alpha_min), r = D - A z ("residual")
    or D / A - z ("expected").  -> (dL/dD, dL/dA, loss, pixels counted, r, the mask of the measured pixels)"""
    D, A, z = (np.asarray(a, np.float64) for a in (D, A, z))
    valid = np.isfinite(z) & (np.where(np.isfinite(z), z, 0.0) > 0)
    if mode == "expected":
        valid &= A >= alpha_min
    zz = np.where(valid, z, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "residual":
            r, dD, dA = D - A * zz, np.ones_like(D), -zz
        else:
            r, dD, dA = D / A - zz, 1.0 / A, -D / (A * A)
    r = np.where(valid, r, 0.0)
    gd = np.where(valid, scale * np.sign(r) * dD, 0.0)
    ga = np.where(valid, scale * np.sign(r) * dA, 0.0)
    return gd, ga, scale * float(np.abs(r).sum()), int(valid.sum()), r, valid


def _sum_by_id(ids, rows, n):
    """index_put_(accumulate=True) (splatter.py:604-613 backward) in float64: rows[j] added to out[ids[j]]."""
    rows = np.asarray(rows, np.float64)
    flat = rows.reshape(len(ids), -1)
    out = np.zeros((n, flat.shape[1]), np.float64)
    if len(ids):
        order = np.argsort(ids, kind="stable")
        sid = np.asarray(ids)[order]
        first = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
        out[sid[first]] = np.add.reduceat(flat[order], first, axis=0)
    return out.reshape((n,) + rows.shape[1:])


# Element-wise gradient tolerance: |got - ref| <= GRAD_RTOL |ref| + GRAD_KAPPA scale, `scale` being the element's own
# conditioning scale from OracleFrame.backward(with_scale=True): the sum over its pixels and (tile, Gaussian) rows of
# |term| (1 + 0.25 x the cancellation inside exp's argument) + 0.05 x (the term with every other internal difference
# replaced by the magnitudes of its operands), pushed through the projection / activation backward in the same way.  A gradient element is a signed sum of thousands of
# fp32 terms, several of them differences of nearly equal numbers (T g.c against g.(C_final - C_run)/(1 - alpha) for
# a Gaussian deep in a tile's list): two correct fp32 evaluations in different orders agree to a number of ulp of
# that scale, however small the sum comes out -- so the tolerance is per element and NOT a fraction of the tensor's
# largest entry.  GRAD_KAPPA = 3e-5 is ~500 ulp of the plain term sum and ~25 ulp of the operand magnitudes (measured
# on the GPU, profiles/r02_a: at 1e-5 every element of cfg2 / cfg3 and all but ONE of the 65 M SH coefficients of cfg4
# pass -- that one, 1.4e-14 against a tensor maximum of ~1e-4 and a scale of 1e-12, sat at 2.05 x); what
# differs between the kernels and the oracle is the summation order, v_exp_f32 / v_rcp_f32 against expf / IEEE
# division, the conic hoisted out of the pixel loop, and the final image each side subtracts its running colour from
# (they agree to ~1e-6).  tools/grad_parity_probe.py prints the measured distribution of err / scale.
GRAD_RTOL = 1e-4
GRAD_KAPPA = 3e-5
GRAD_L2 = 2e-5  # ||got - ref||_2 / ||ref||_2 per tensor
# Independent of the oracle-supplied scale, and CALIBRATED rather than fitted: the PURE
# relative error |got - truth| / |truth| against a DOUBLE-precision evaluation of the same formulas
# (OracleFrame.backward_f64), over the elements above 1e-6 of the tensor's largest entry, compared quantile by quantile
# with the error the REFERENCE's own fp32 arithmetic has against that same truth:
#   * at the size where the reference's kernels are well defined, their outputs are committed
#     (tests/golden/calib_*.npz) and the HIP kernels' error quantiles are bounded by CALIB_K x theirs
#     (tests/test_grad_calibration.py) -- where the same file shows that the ORACLE's error distribution is the
#     reference kernels' (same fp32 terms; quantiles within a factor 2, measured within 20 %);
#   * at full size (tests/test_gpu_frame.py) the reference kernel is not defined (its chunk defect), and the oracle
#     -- fp32 terms in the reference's expression order, accumulated in double: never WORSE than the reference's
#     fp32 shuffles / atomics -- stands in for it: assert_error_no_worse_than.
# What the reference's own arithmetic achieves (calib fixtures, lists <= 166): median ~1e-6, 99.9th percentile 1e-4 ...
# 5e-4, maximum up to 1.8e-2 -- percent-level single elements are a property of fp32 on these sums, not of a kernel.
CALIB_QS = (0.5, 0.9, 0.99, 0.999, 1.0)
CALIB_K = 4.0  # error quantile (median ... 99.9 %) of a HIP kernel <= CALIB_K x the same quantile of the reference arithmetic's error
CALIB_K_MAX = 8.0  # the MAXIMUM of the relative error: a one-element statistic of an element that is the small difference of
#                    large terms -- which element that is, and how lucky the reference was on it, differs between evaluations
#                    (measured over the golden-size cases, round 6: quantiles up to 99.9 % within 3.6 x, maxima within 5.9 x)
CALIB_K_ELEM = 6.0  # per element: e_hip <= CALIB_K_ELEM x max(e_ref, the reference's 99.9th-percentile error on sums of that magnitude)
#                      (measured: worst element 4.7 x, 99.9th percentile 0.8 - 1.1 x)


def rel_error_quantiles(got, truth, qs=CALIB_QS, floor=1e-6):
    """Quantiles of |got - truth| / |truth| over the elements with |truth| > floor x max |truth|."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    a = np.abs(truth)
    big = a > floor * (a.max() if a.size else 0.0)
    if not big.any():
        return [0.0] * len(qs)
    r = np.abs(got - truth)[big] / a[big]
    return [float(np.quantile(r, q)) for q in qs]


def elementwise_error_ratio(got, ref, truth, scale):
    """Element by element: e_got / max(e_ref, F x scale) -> (99.9th percentile, maximum, F, the same F for `got`).
    `scale` is the element's term-magnitude sum (the oracle's conditioning scale with scale_w = 0) and F the REFERENCE
    evaluation's own tail error per unit of scale, the 99.9th percentile of e_ref / scale over the tensor: where the
    reference happened to round luckily, an element is held to what the reference's arithmetic delivers at its 99.9th
    percentile on sums of that magnitude -- not to that luck.  (Errors of two independent fp32 evaluations are not
    correlated element by element: against max(e_ref, one ulp of scale) the ORACLE passes with 1.5, because it shares
    the reference's per-term arithmetic, while any kernel with another exp / rcp / summation order sits at 5 - 25.)"""
    got, ref, truth, scale = (np.asarray(a, np.float64).ravel() for a in (got, ref, truth, scale))
    e_got, e_ref = np.abs(got - truth), np.abs(ref - truth)
    pos = scale > 0
    F = float(np.quantile(e_ref[pos] / scale[pos], 0.999)) if pos.any() else 0.0
    F_got = float(np.quantile(e_got[pos] / scale[pos], 0.999)) if pos.any() else 0.0
    ratio = e_got / np.maximum(np.maximum(e_ref, F * scale), 1e-300)
    return float(np.quantile(ratio, 0.999)), float(ratio.max()), F, F_got


def assert_error_no_worse_than(grads, truth, ref, what="", k=CALIB_K):
    """Five parameter gradients `grads` and the reference arithmetic's `ref` (the oracle's, fp32 terms) against the
    double-precision `truth`: every quantile of CALIB_QS of the HIP error is within k x the reference arithmetic's.
    -> {name: (hip quantiles, reference quantiles)}"""
    report = {}
    for g, name in zip(grads, ("pos", "quat", "scale", "opa", "rgb")):
        qh = rel_error_quantiles(np.asarray(g), truth[name])
        qr = rel_error_quantiles(ref[name], truth[name])
        report[name] = (qh, qr)
        for a, b, q in zip(qh, qr, CALIB_QS):
            assert a <= (CALIB_K_MAX if q == 1.0 else k) * b, (what, name, "quantile", q, "hip error", a,
                                                               "reference arithmetic's error", b)
    return report


def assert_rows_error_no_worse_than(got, truth, ref, what="", k=CALIB_K):
    """The same statement for the four (tile, Gaussian)-row gradients of draw_backward (pos x / y, rgb, opa, cov)."""
    report = {}
    for g, t, r, name in zip(got, truth, ref, ROW_NAMES):
        cut = (lambda a: np.asarray(a).reshape(np.asarray(t).shape)[:, :2]) if name == "pos" else \
            (lambda a: np.asarray(a).reshape(np.asarray(t).shape))
        qh, qr = rel_error_quantiles(cut(g), cut(t)), rel_error_quantiles(cut(r), cut(t))
        report[name] = (qh, qr)
        for a, b, q in zip(qh, qr, CALIB_QS):
            assert a <= (CALIB_K_MAX if q == 1.0 else k) * b, (what, "rows", name, "quantile", q, "hip error", a,
                                                               "reference arithmetic's error", b)
    return report


# Entries 14 orders of magnitude below the tensor's largest are compared up to this floor: they are sums of products
# whose intermediates underflow in fp32 (the transcendental unit flushes subnormal operands, the CPU oracle keeps
# them) or whose dL/dimage factor is itself a rounding residue of image - target.  Measured at cfg4 (65 M SH
# coefficients): with the floor at 1e-16 exactly one element (ref 2.0e-18 against a tensor maximum of ~1e-4) sat at
# 2.2 x its tolerance; nothing an optimiser sees: torch.optim.Adam (train.py:56) adds eps = 1e-8 to sqrt(v), so a 1e-18 gradient moves nothing.
GRAD_FLOOR_REL = 1e-14
GRAD_FLOOR = 1e-30


def grad_close(got, ref, scale, rtol=GRAD_RTOL, kappa=GRAD_KAPPA):
    """-> (ok, worst ratio err / tol, index of the worst element, fraction of elements within rtol |ref| alone)."""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    err = np.abs(got - ref)
    tol = rtol * np.abs(ref) + kappa * scale + GRAD_FLOOR + GRAD_FLOOR_REL * (np.abs(ref).max() if ref.size else 0.0)
    bad = err > tol
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    worst = int(np.argmax(ratio)) if ratio.size else 0
    pure = float(np.mean(err <= rtol * np.abs(ref))) if err.size else 1.0
    return (not bool(bad.any()) and bool(np.isfinite(got).all())), float(ratio.flat[worst]) if ratio.size else 0.0, \
        np.unravel_index(worst, ratio.shape) if ratio.size else (), pure


def assert_grads_close(grads, ref, scale, what="", rtol=GRAD_RTOL, kappa=GRAD_KAPPA, l2=GRAD_L2):
    """grads: five arrays (pos, quat, scale, opa, rgb) -> element-wise check of each against the oracle + a relative
    L2 bound per tensor + bounds on the pure relative error.  Returns {name: (worst err / tol, fraction of elements inside
    rtol |ref| alone, rel. L2, worst pure relative error over the elements above 1e-6 of the tensor's maximum, its 99.9th
    percentile)}."""
    report = {}
    for g, name in zip(grads, ("pos", "quat", "scale", "opa", "rgb")):
        g = np.asarray(g)
        ok, worst, where, pure = grad_close(g, ref[name], scale[name], rtol, kappa)
        rl2 = float(np.linalg.norm(g.astype(np.float64) - ref[name]) / (np.linalg.norm(ref[name].astype(np.float64)) + 1e-300))
        # worst PURE relative error |got - ref| / |ref| over the elements above 1e-6 of the tensor's largest (reported;
        # the asserted oracle-independent statement is assert_error_no_worse_than, against a double-precision truth)
        r64 = np.abs(np.asarray(ref[name], np.float64))
        big = r64 > 1e-6 * (r64.max() if r64.size else 0.0)
        rels = np.abs(g.astype(np.float64) - ref[name])[big] / r64[big] if big.any() else np.zeros(1)
        rel_big = float(rels.max())
        rel_p999 = float(np.quantile(rels, 0.999))
        report[name] = (round(worst, 3), round(pure, 5), rl2, rel_big, rel_p999)
        assert ok, (what, name, "worst err/tol", worst, "at", where, "got", float(g[where]), "ref",
                    float(ref[name][where]), "scale", float(scale[name][where]))
        assert rl2 <= l2, (what, name, "relative L2 error", rl2)
    return report


ROW_NAMES = ("pos", "rgb", "opa", "cov")


def assert_rows_close(got, ref, scale, what="", rtol=GRAD_RTOL, kappa=GRAD_KAPPA, l2=GRAD_L2):
    """The four (tile, Gaussian)-row gradients of draw_backward (pos, rgb, opa, cov -- renderer.py:46-58) against the
    oracle's, ELEMENT BY ELEMENT in units of each element's conditioning scale (oracle.draw_backward(with_scale=True)),
    plus a relative L2 bound per tensor: the standard of the frame path's parameter gradients (assert_grads_close)
    applied at the reference API's own boundary.  -> {name: (worst err / tol, fraction within rtol |ref| alone, rel. L2)}"""
    report = {}
    for g, r, sc, name in zip(got, ref, scale, ROW_NAMES):
        g = np.asarray(g).reshape(np.asarray(r).shape)
        ok, worst, where, pure = grad_close(g, r, sc, rtol, kappa)
        rl2 = float(np.linalg.norm(g.astype(np.float64) - r) / (np.linalg.norm(np.asarray(r, np.float64)) + 1e-300))
        report[name] = (round(worst, 3), round(pure, 5), rl2)
        assert ok, (what, name, "worst err/tol", worst, "at", where, "got", float(g[where]), "ref", float(r[where]),
                    "scale", float(sc[where]))
        assert rl2 <= l2, (what, name, "relative L2 error", rl2)
    return report


def robust_padded_grad(of, gpad, band=2e-5):
    """dL/d(padded image) zeroed on the pixels whose early-stop decision is not robust in fp32 (OracleFrame.robust_grad_image
    for the padded image the reference API's draw works on).  -> (gpad, #pixels zeroed)"""
    grid = of.grid
    amb = oracle.draw_ambiguous(of.s_pos, of.s_opa, of.s_cov, of.accum, grid.padded_height, grid.padded_width,
                                grid.focal_x, grid.focal_y, band)
    keep = ~amb[:, :, None].astype(bool)
    return np.ascontiguousarray(gpad * keep, np.float32), int(amb.sum())


def rel_err(a, b):
    """max |a-b| / (max |b| + tiny): scale-aware error for gradient tensors."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def to_torch(scene: Scene, device, requires_grad=False):
    import torch

    out = []
    for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        t.requires_grad_(requires_grad)
        out.append(t)
    return out
