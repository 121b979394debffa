"""A CPU model of the temporal occlusion cull's trim rule (GS_FRAME_OCCLUSION_CULL), on top of the oracle.

What the device does (csrc/gs_frame_layout.h, strip_common.h: walk_strips<CUT>, tile_sort.hip: strip_sort_kernel):
  * the compositing of frame k leaves, per tile, cut = depth of the last Gaussian it composited x (1 + GS_CUT_MARGIN) when all
    the tile's pixels had stopped inside (or exactly at the end of) its list, GS_NO_CUT otherwise;
  * frame k + 1 lists a Gaussian, per (tile row, strip of 8 tiles), in the tiles [first, last] of its run whose cut does not
    lie in front of it -- the run is trimmed at its two ENDS only, so an interior tile whose cut lies in front of the
    Gaussian still lists it.  A trimmed list is therefore every pair with depth <= cut ("the prefix") plus some deeper ones;
  * a tile whose walk is not covered by the prefix raises the fallback, and the frame is rendered again from the full lists.

The model takes the full per-tile lists from ``OracleFrame`` and restates exactly that in NumPy: the per-tile stop step, the
cut table, its 3 x 3 dilation, the end-trimmed lists and their image (oracle.draw).  Depths compare as their fp32 bits, like
on the device.  rgb scenes only (the geometry is what is modelled).

The crafted scene (``crafted_scene``): 256 x 96 pixels = 16 x 6 tiles = two strips per tile row.  An opaque occluder over the
3 x 3 block of tiles (rows 2..4, columns 2..4), three small Gaussians behind it inside tile (3, 3) alone, and a wall of huge
Gaussians behind everything.  With the occluder's cuts in the table the small ones are trimmed, while the wall's run in strip
0 keeps its ends (tiles 0..1 and 5..7) and so stays listed in the block.  When the occluder fades, tile (3, 3) composites the
wall WITHOUT the small Gaussians in front of it, saturates on it, and nothing ends live.
"""
from __future__ import annotations

import numpy as np

import oracle
from gs_scene import Scene, make_camera
from gs_testutil import OracleFrame

NO_CUT = np.uint32(0xFFFFFFFF)       # GS_NO_CUT
CUT_MARGIN = np.float32(0.0625)      # GS_CUT_MARGIN
STRIP_W = 8                          # GS_STRIP_W
DILATE = np.float32(1.375)           # GS_CUT_DILATE_SCALE
DILATE_NEAR = np.float32(1.125)      # GS_CUT_DILATE_SCALE_NEAR

W, H, FX = 256, 96, 192.0
N_OCC, N_SMALL, N_WALL = 8, 3, 8
OCC, SMALL, WALL = slice(0, 8), slice(8, 11), slice(11, 19)
BLOCK = [(r, c) for r in (2, 3, 4) for c in (2, 3, 4)]  # (tile row, tile column) under the occluder
SMALL_TILE = (3, 3)
SMALL_PX = (56, 56)


def _at(px, py, z):
    return [(px - W / 2) / FX * z, (py - H / 2) / FX * z, z]


def crafted_scene(wall: bool = True) -> Scene:
    """19 isotropic Gaussians (11 without the wall), quaternion (1, 0, 0, 0), opacity logit 8, raw scale sigma_px z / fx."""
    rows = []  # (position, sigma in pixels, colour logits)
    rows += [(_at(56, 56, 2.0 + 0.001 * k), 40.0, (-3, -3, 3)) for k in range(N_OCC)]
    rows += [(_at(56, 56, 4.0 + 0.001 * k), 3.0, (4, -4, -4)) for k in range(N_SMALL)]
    if wall:
        rows += [(_at(64, 48, 8.0 + 0.001 * k), 400.0, (-3, 3, -3)) for k in range(N_WALL)]
    n = len(rows)
    pos = np.array([r[0] for r in rows], np.float32)
    scale = np.array([[r[1] * r[0][2] / FX] * 3 for r in rows], np.float32)
    quat = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opa = np.full(n, 8.0, np.float32)
    rgb = np.array([r[2] for r in rows], np.float32)
    return Scene(pos, quat, scale, opa, rgb)


def crafted_camera(shift_px: float = 0.0):
    """The crafted scene's camera, yawed so that the image content moves by about ``shift_px`` pixels."""
    return make_camera(W, H, yaw_deg=float(np.degrees(shift_px / FX)))


def faded(scene: Scene) -> Scene:
    """The edit: the occluder's opacity logit becomes -8 (alpha 3e-4)."""
    s = Scene(scene.pos.copy(), scene.quat.copy(), scene.scale.copy(), scene.opa.copy(), scene.rgb.copy())
    s.opa[OCC] = -8.0
    return s


def moved_out(scene: Scene) -> Scene:
    """The other edit: the occluder leaves the frustum (far to the side of the image)."""
    s = Scene(scene.pos.copy(), scene.quat.copy(), scene.scale.copy(), scene.opa.copy(), scene.rgb.copy())
    s.pos[OCC, 0] += 100.0
    return s


class TrimModel:
    """One frame of ``scene`` under ``cam``: full lists, stop steps, cuts, trimmed lists, images."""

    def __init__(self, scene: Scene, cam):
        assert not scene.use_sh, "the model draws rgb scenes"
        self.of = of = OracleFrame(scene, cam)
        g = of.grid
        self.ntx, self.nty, self.T = g.n_tile_x, g.n_tile_y, g.n_tile_x * g.n_tile_y
        assert (g.padded_width, g.padded_height) == (16 * self.ntx, 16 * self.nty)
        self.lists = [np.asarray(of.ids[of.accum[t]:of.accum[t + 1]], np.int64) for t in range(self.T)]
        self.dbits = np.ascontiguousarray(of.pos_i[:, 2], np.float32).view(np.uint32)  # the sort key: bits of |p_c|
        # a faint, far Gaussian that covers the frame: row n of the arrays below
        n = scene.n
        self._pos = np.concatenate([of.pos_i, [[0.0, 0.0, 1e6]]]).astype(np.float32)
        self._cov = np.concatenate([of.cov.reshape(-1, 4), [[1e4, 0.0, 0.0, 1e4]]]).astype(np.float32)
        self._opa = np.concatenate([of.opa_act, [0.02]]).astype(np.float32)
        self._col = np.concatenate([of.col_act, [[1.0, 1.0, 1.0]]]).astype(np.float32)
        self._sentinel = n

    def tile(self, row, col):
        return row * self.ntx + col

    def pairs(self, lists):
        return int(sum(len(l) for l in lists))

    # ------------------------------------------------------------------ drawing
    def _draw(self, lists, colours, sentinel=False):
        if sentinel:
            lists = [np.concatenate([l, [self._sentinel]]) for l in lists]
        ids = np.concatenate(lists).astype(np.int64) if self.pairs(lists) else np.zeros(0, np.int64)
        accum = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        g = self.of.grid
        return oracle.draw(self._pos[ids], colours[ids], self._opa[ids], self._cov[ids], accum, g.padded_height,
                           g.padded_width, g.focal_x, g.focal_y, fast=True)

    def image(self, lists):
        """[H, W, 3], clamped and cropped like the renderer's."""
        return self.of.grid.crop(np.clip(self._draw(lists, self._col), 0, 1))

    def tile_of_pixels(self, mask):
        """[H, W] bool -> set of (tile row, tile column) that hold a True pixel (the crafted frames are not padded)."""
        assert mask.shape == (16 * self.nty, 16 * self.ntx)
        per = mask.reshape(self.nty, 16, self.ntx, 16).any(axis=(1, 3))
        return {(int(r), int(c)) for r, c in zip(*np.nonzero(per))}

    # ------------------------------------------------------------------ where a tile stops
    def _stopped(self, lists, k):
        """Per tile: has every pixel stopped after the first k[t] entries of its list?  A pixel has stopped iff appending
        the sentinel (alpha 0.02) leaves its alpha unchanged: the reference's test is `T < 1e-4` BEFORE a Gaussian is
        evaluated, so a pixel at T = 1.4e-4 behind an opaque Gaussian is live however close its alpha is to one."""
        pre = [l[:kk] for l, kk in zip(lists, k)]
        ones = np.ones_like(self._col)
        a, b = self._draw(pre, ones)[:, :, 0], self._draw(pre, ones, sentinel=True)[:, :, 0]
        live = (a != b).reshape(self.nty, 16, self.ntx, 16).any(axis=(1, 3)).ravel()
        return ~live

    def stop_steps(self, lists, live_every: int = 1):
        """[T] int: the number of Gaussians a tile composites before all its pixels have stopped, -1 for a tile that reaches
        the end of its list with a live pixel (an empty list included).  ``live_every``: the device tests a tile's liveness
        in front of every 8th (rgb) or 4th (SH, aux) Gaussian of a chunk and at the end of the list, so ITS stop step is the
        model's rounded up to that grid, the list's length at most."""
        n = np.array([len(l) for l in lists], np.int64)
        end = self._stopped(lists, n) & (n > 0)
        lo, hi = np.zeros(self.T, np.int64), n.copy()  # not stopped after lo (nothing composited: T = 1), stopped after hi
        lo[~end] = n[~end]
        while (hi - lo > 1).any():
            mid = (lo + hi) // 2
            s = self._stopped(lists, mid)
            hi, lo = np.where(s, mid, hi), np.where(s, lo, mid)
        hi = np.minimum((hi + live_every - 1) // live_every * live_every, n)
        return np.where(end, hi, -1)

    def last_depth(self, lists, stop):
        """[T] uint32: depth bits of the last Gaussian a tile composited; NO_CUT (the largest value) where it ended live."""
        return np.array([self.dbits[l[s - 1]] if s > 0 else NO_CUT for l, s in zip(lists, stop)], np.uint32)

    def cuts(self, lists, stop):
        """The cut table the compositing of these lists leaves behind."""
        d = self.last_depth(lists, stop)
        c = (d.view(np.float32) * (np.float32(1) + CUT_MARGIN)).astype(np.float32).view(np.uint32)
        return np.where(np.asarray(stop) > 0, c, NO_CUT).astype(np.uint32)

    def dilate(self, cut, factor):
        """GS_FRAME_CULL_DILATE: the largest cut of every tile's 3 x 3 neighbourhood, pushed back by ``factor`` in depth."""
        c = np.asarray(cut, np.uint32).reshape(self.nty, self.ntx)
        p = np.pad(c, 1, mode="edge")
        m = np.max([p[j:j + self.nty, i:i + self.ntx] for j in range(3) for i in range(3)], axis=0).astype(np.uint32)
        with np.errstate(invalid="ignore"):
            d = (m.view(np.float32) * np.float32(factor)).astype(np.float32).view(np.uint32)
        return np.where(m == NO_CUT, NO_CUT, d).ravel().astype(np.uint32)

    # ------------------------------------------------------------------ the trim
    def trimmed_lists(self, cut):
        """This frame's lists under the cut table ``cut`` (plain or dilated): per Gaussian, tile row and strip, the tiles from
        the first to the last of its run whose cut does not lie in front of it."""
        n = self.of.scene.n
        listed = np.zeros((n, self.nty, self.ntx), bool)
        for t, l in enumerate(self.lists):
            listed[l, t // self.ntx, t % self.ntx] = True
        keep = listed & (self.dbits[:, None, None] <= np.asarray(cut, np.uint32).reshape(1, self.nty, self.ntx))
        out = np.zeros_like(listed)
        for x0 in range(0, self.ntx, STRIP_W):
            k = keep[:, :, x0:x0 + STRIP_W]
            w = k.shape[2]
            lo, hi = k.argmax(2), w - 1 - k[:, :, ::-1].argmax(2)
            x = np.arange(w)
            out[:, :, x0:x0 + w] = k.any(2)[..., None] & (x >= lo[..., None]) & (x <= hi[..., None])
        assert not (out & ~listed).any(), "a Gaussian's tiles in a tile row are one run"
        return [l[out[l, t // self.ntx, t % self.ntx]] for t, l in enumerate(self.lists)]

    # ------------------------------------------------------------------ the fallback rules
    def ends_live(self, lists, stop, cut):
        """Tiles the rule `a tile with a cut reached the end of its trimmed list with a live pixel` names."""
        return {(t // self.ntx, t % self.ntx) for t in range(self.T) if cut[t] != NO_CUT and stop[t] < 0}

    def past_cut(self, lists, stop, cut):
        """Tiles with a cut whose last composited Gaussian lies behind it (depth bits exceed the cut), or that ended live: a
        walk the prefix {d <= cut} does not cover."""
        d = self.last_depth(lists, stop)
        return {(t // self.ntx, t % self.ntx) for t in range(self.T) if cut[t] != NO_CUT and d[t] > cut[t]}
