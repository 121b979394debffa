"""Restatement of the per-Gaussian contribution statistics (include/gs_abi.h, gs_frame_contrib) in torch float64 on the CPU.

From a frame's lists and records -- ``sorted_ids`` [M], ``tile_ranges`` [T,2], ``rec_geom`` [N,4] = (x, y, depth, sigmoid(opa)),
``rec_cov`` [N,4] = (a, b, c, d): what ``FrameRenderer.debug_views()`` shows, or the same arrays of an ``OracleFrame`` -- and the
frame geometry, every tile is composited as the oracle's K7 does (oracle/gs_oracle.c, gso_draw): the pixel stops at the first
Gaussian that finds its transmittance below ``stop`` (the test comes BEFORE the Gaussian is composited), w = alpha T,
T <- T (1 - alpha), alpha = sigmoid(opa) 2^-(A dx^2 - B dx dy + C dy^2) with the conic by gs_conic's formula
(csrc/gs_common.h: k = log2(e) / (2 det + 1e-14), A = d k, B = (b + c) k, C = a k).  Pixels of the padded border count for
nothing in the statistics (``w`` itself is returned for all 256 pixels of a tile).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

LOG2E = 1.4426950408889634
TILE = 16


@dataclass
class ContribRef:
    w: torch.Tensor            # [M,256] float64: w of pair j (sorted order) at tile pixel 16 row + column
    pair_tile: torch.Tensor    # [M] tile of pair j
    inside: torch.Tensor       # [T,256] bool: the tile pixel lies inside the cropped image
    weight_sum: torch.Tensor   # [N] float64
    weight_max: torch.Tensor   # [N] float64
    pixels: torch.Tensor       # [N] int64: image pixels with w >= w_min
    views: torch.Tensor        # [N] int64: pixels > 0
    tile_pixels: torch.Tensor  # [N] int64: image pixels in the tiles the Gaussian is listed in
    alpha_map: torch.Tensor    # [padH,padW] float64: sum over Gaussians of w (the alpha map of the padded frame)


def frame_geometry(width: int, height: int):
    pad_w, pad_h = (width + TILE - 1) // TILE * TILE, (height + TILE - 1) // TILE * TILE
    return pad_w, pad_h, pad_w // TILE, pad_h // TILE, (pad_h - height) // 2, (pad_w - width) // 2


def composite(sorted_ids, tile_ranges, rec_geom, rec_cov, width: int, height: int, focal_x: float, focal_y: float,
              stop: float = 1e-4, w_min: float = 1.0 / 255.0) -> ContribRef:
    ids = torch.as_tensor(sorted_ids).to(torch.int64).cpu()
    ranges = torch.as_tensor(tile_ranges).to(torch.int64).cpu().reshape(-1, 2)
    geom = torch.as_tensor(rec_geom).to(torch.float64).cpu()
    cov = torch.as_tensor(rec_cov).to(torch.float64).cpu()
    n, m = geom.shape[0], ids.shape[0]
    pad_w, pad_h, ntx, nty, crop_top, crop_left = frame_geometry(width, height)
    n_tiles = ntx * nty
    assert ranges.shape[0] == n_tiles, (ranges.shape, n_tiles)
    det = cov[:, 0] * cov[:, 3] - cov[:, 1] * cov[:, 2]
    k = LOG2E / (2.0 * det + 1e-14)
    conic = torch.stack([cov[:, 3] * k, (cov[:, 1] + cov[:, 2]) * k, cov[:, 0] * k], 1)
    lx = torch.arange(256) % TILE
    ly = torch.arange(256) // TILE
    w = torch.zeros(m, 256, dtype=torch.float64)
    pair_tile = torch.zeros(m, dtype=torch.int64)
    inside = torch.zeros(n_tiles, 256, dtype=torch.bool)
    alpha_map = torch.zeros(pad_h, pad_w, dtype=torch.float64)
    for t in range(n_tiles):
        tx, ty = t % ntx, t // ntx
        ix, iy = tx * TILE + lx, ty * TILE + ly
        inside[t] = (ix - crop_left >= 0) & (ix - crop_left < width) & (iy - crop_top >= 0) & (iy - crop_top < height)
        px = (ix.to(torch.float64) + 0.5 - pad_w // 2) / focal_x
        py = (iy.to(torch.float64) + 0.5 - pad_h // 2) / focal_y
        T = torch.ones(256, dtype=torch.float64)
        live = torch.ones(256, dtype=torch.bool)
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        pair_tile[s:e] = t
        for j in range(s, e):
            g = int(ids[j])
            live = live & ~(T < stop)  # K7: `if (accum < 0.0001) break;` in front of the Gaussian
            if not bool(live.any()):
                break
            dx, dy = px - geom[g, 0], py - geom[g, 1]
            q = conic[g, 0] * dx * dx - conic[g, 1] * dx * dy + conic[g, 2] * dy * dy
            alpha = geom[g, 3] * torch.exp2(-q)
            wj = torch.where(live, alpha * T, torch.zeros_like(T))
            w[j] = wj
            T = torch.where(live, T * (1.0 - alpha), T)
        alpha_map[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = w[s:e].sum(0).reshape(TILE, TILE)
    win = w * inside[pair_tile].to(torch.float64)
    weight_sum = torch.zeros(n, dtype=torch.float64).index_add_(0, ids, win.sum(1))
    weight_max = torch.zeros(n, dtype=torch.float64)
    if m:
        weight_max.scatter_reduce_(0, ids, win.max(1).values, reduce="amax", include_self=True)
    pixels = torch.zeros(n, dtype=torch.int64).index_add_(0, ids, (win >= w_min).sum(1))
    tile_pixels = torch.zeros(n, dtype=torch.int64).index_add_(0, ids, inside[pair_tile].sum(1))
    return ContribRef(w, pair_tile, inside, weight_sum, weight_max, pixels, (pixels > 0).to(torch.int64), tile_pixels,
                      alpha_map)


def pixel_counts(ref: ContribRef, n: int, sorted_ids, w_min: float) -> torch.Tensor:
    """[N] int64: image pixels with w >= w_min, from a finished restatement (another floor, the same compositing)."""
    ids = torch.as_tensor(sorted_ids).to(torch.int64).cpu()
    win = ref.w * ref.inside[ref.pair_tile].to(torch.float64)
    return torch.zeros(n, dtype=torch.int64).index_add_(0, ids, (win >= w_min).sum(1))


def from_oracle_frame(of, stop: float = 1e-4, w_min: float = 1.0 / 255.0) -> ContribRef:
    """The restatement on the lists and records of a ``gs_testutil.OracleFrame`` (no GPU)."""
    import numpy as np

    grid = of.grid
    n = of.scene.n
    geom = np.zeros((n, 4), np.float64)
    geom[:, 0:2] = of.pos_i[:, 0:2]
    geom[:, 3] = of.opa_act
    accum = np.asarray(of.accum, np.int64)
    ranges = np.stack([accum[:-1], accum[1:]], 1)
    return composite(of.ids, ranges, geom, of.cov.reshape(-1, 4), of.cam.width, of.cam.height, grid.focal_x, grid.focal_y,
                     stop=stop, w_min=w_min)


def from_renderer(r, stop: float = 1e-4, w_min: float = 1.0 / 255.0) -> ContribRef:
    """The restatement on the lists and records of a FrameRenderer's last forward (``debug_views()``)."""
    v = r.debug_views()
    f = r._frame
    return composite(v["sorted_ids"].cpu(), v["tile_ranges"].cpu(), v["rec_geom"].cpu(), v["rec_cov"].cpu(), int(f.width),
                     int(f.height), float(f.focal_x), float(f.focal_y), stop=stop, w_min=w_min)
