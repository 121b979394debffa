"""Image pyramids for coarse-to-fine camera tracking: the level targets (``Pyramid``, on gs_pyramid_down -- csrc/pyramid.hip,
include/gs_abi.h) and the level cameras (``level_camera``).

Level l of a frame is gs_pyramid_down applied l times: colour box-filtered 2 x 2 per level, and a range map in which a coarse
pixel is measured where at least ``min_valid`` of its four fine pixels are and -- with ``edge_rel`` >= 0 -- their largest
range is at most (1 + edge_rel) x their smallest; its value is the mean of the measured ones, an unmeasured pixel is 0.  The
mean of four ranges along four slightly different rays approximates the range along the coarse pixel's own ray to second
order: targets for tracking, not for seeding or mapping.
"""
from __future__ import annotations

import copy
import ctypes as C
from typing import List, Optional, Tuple

import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream
from gs_geometry import principal_point_default

MAX_LEVELS = _lib.GS_PYRAMID_MAX_LEVELS


def level_sizes(height: int, width: int, levels: int) -> List[Tuple[int, int]]:
    """[(H_l, W_l)] for l = 0..levels; refuses ``levels`` outside 0..GS_PYRAMID_MAX_LEVELS and a size that 2^levels does not
    divide.  Host only."""
    height, width, levels = int(height), int(width), int(levels)
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels must be 0..{MAX_LEVELS} (GS_PYRAMID_MAX_LEVELS), got {levels}")
    if height <= 0 or width <= 0 or height % (1 << levels) or width % (1 << levels):
        raise ValueError(f"a {width} x {height} frame has no level {levels}: 2^{levels} = {1 << levels} does not divide it")
    return [(height >> l, width >> l) for l in range(levels + 1)]


def level_camera(camera, level: int):
    """The camera of pyramid level ``level``: a copy with ``width >> level``, ``height >> level``, the focal lengths and the
    principal point divided by 2^level -- the exact pinhole relation for pixels that cover [i, i+1): the point at fine pixel
    coordinate u lies at u / 2^level.  The full-resolution principal point is the camera's ``cx`` / ``cy`` where it has one,
    else the renderer's own centre (gs_geometry.principal_point_default).  An odd coarse size then sits half a pixel off that
    level's own centre and takes the renderer's principal-point path; an even-sized centred camera gets an offset of (0, 0)
    at every level and runs the kernels it always ran.  Level 0 is the camera itself, unchanged (it does not gain a ``cx``)."""
    level = int(level)
    if not 0 <= level <= MAX_LEVELS:
        raise ValueError(f"level must be 0..{MAX_LEVELS} (GS_PYRAMID_MAX_LEVELS), got {level}")
    if level == 0:
        return camera
    level_sizes(camera.height, camera.width, level)
    cx0, cy0 = principal_point_default(camera.width, camera.height)
    cx, cy = getattr(camera, "cx", None), getattr(camera, "cy", None)
    f = float(1 << level)
    c = copy.copy(camera)
    c.width, c.height = int(camera.width) >> level, int(camera.height) >> level
    c.focal_x, c.focal_y = camera.focal_x / f, camera.focal_y / f
    c.cx = (cx0 if cx is None else float(cx)) / f
    c.cy = (cy0 if cy is None else float(cy)) / f
    return c


class Pyramid:
    """``Pyramid(height, width, levels, device)`` owns the buffers of levels 1..``levels``, allocated once.  ``build(image,
    range_map=None)`` issues ``levels`` launches of gs_pyramid_down on the current stream -- no host synchronisation, no
    allocation -- and returns ``(images, ranges)``, lists indexed by level; entry 0 is the caller's tensors themselves
    (``ranges`` holds None throughout for an RGB-only frame).  The buffers are overwritten by the next ``build``.

    The defaults have no evidence behind them: ``min_valid`` 2 means at least half of a footprint is measured, so holes in the
    range map do not erode a whole pixel per level; ``edge_rel`` 0.1 is arbitrary (< 0 switches the edge test off)."""

    def __init__(self, height: int, width: int, levels: int, device="cuda", min_valid: int = 2, edge_rel: float = 0.1):
        self.sizes = level_sizes(height, width, levels)
        self.levels = int(levels)
        self.H, self.W = self.sizes[0]
        if not 1 <= int(min_valid) <= 4:
            raise ValueError(f"min_valid must be 1..4, got {min_valid}")
        if edge_rel != edge_rel:
            raise ValueError("edge_rel must not be NaN (negative: the edge test is off)")
        self.device = require_hip(device, "Pyramid")
        self._opts = _lib.GsPyramidOpts(int(min_valid), float(edge_rel))
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)  # noqa: E731
        self._images = [None] + [new(h, w, 3) for h, w in self.sizes[1:]]
        self._ranges = [None] + [new(h, w) for h, w in self.sizes[1:]]

    def build(self, image: torch.Tensor, range_map: Optional[torch.Tensor] = None):
        check_tensor("image", image, (self.H, self.W, 3))
        if range_map is not None:
            check_tensor("range_map", range_map, (self.H, self.W))
        images = [image] + self._images[1:]
        ranges = [range_map] + (self._ranges[1:] if range_map is not None else [None] * self.levels)
        if self.levels:
            with torch.cuda.device(self.device):
                s = stream()
                for l in range(self.levels):
                    h, w = self.sizes[l]
                    _lib.call("gs_pyramid_down", images[l].data_ptr(), ranges[l].data_ptr() if range_map is not None else None,
                              h, w, C.byref(self._opts), images[l + 1].data_ptr(),
                              ranges[l + 1].data_ptr() if range_map is not None else None, s)
        return images, ranges
