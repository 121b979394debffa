"""Seeding from RGB-D frames: new Gaussians where a depth camera saw a surface the model does not explain.

``seed_from_depth(image, depth, camera, rendered=(depth_map, alpha_map))`` back-projects the measured pixels of a view that
the current model leaves open -- rendered alpha below ``alpha_thresh``, or a measurement in front of the expected depth by
more than ``front_rel`` -- and returns one Gaussian per such pixel: at the measured point on the renderer's own ray through
the pixel centre, isotropic with sigma = ``scale_factor`` lattice steps at that depth, opacity ``opa_init``, the pixel's
colour (include/gs_abi.h, gs_seed_classify / gs_seed_apply; csrc/seed.hip).  Without ``rendered`` the model is empty and
every measured pixel of the ``stride`` lattice is taken: this is how a fit on an RGB-D sequence starts, which has no COLMAP
points.  Three HIP launches and one host read of the count in between (a control step, like ``gs_densify.adaptive_control``);
the rows come in row-major pixel order, bitwise repeatable.  ``gs_train.Trainer.seed_from_view`` is the hook that extends the
Gaussian set of a running fit by a view.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace
from gs_geometry import pose_ctypes, principal_point_offset

SCALE_ACT = {"abs": 0, "exp": 1}
# opa_init > alpha_thresh: a pixel that was seeded has A >= opa_init at its centre from its own Gaussian alone, so the
# same view does not select it a second time
# front_rel / opa_init: the seeded pixel's own Gaussian leaves at most 1 - opa_init of the ray to what lies behind it, so the
# "in front" test z A < (1 - front_rel) D can fire again only across a depth edge with a far / near ratio beyond
# (1 - opa_init (1 - front_rel)) / ((1 - opa_init) (1 - front_rel)) = 3.5, and only where no seeded neighbour covers the pixel.
# scale_factor 0.7: the four seeds around a lattice cell's corner still close it (alpha 0.95 there at opa_init 0.9).
DEFAULTS = dict(stride=1, alpha_thresh=0.5, front_rel=0.2, scale_factor=0.7, opa_init=0.9)
ROW_SHAPES = ((3,), (4,), (3,), (), None)  # pos, quat, scale, opa, rgb (color_dim)


def seed_options(stride: int = DEFAULTS["stride"], alpha_thresh: float = DEFAULTS["alpha_thresh"],
                 front_rel: float = DEFAULTS["front_rel"], scale_factor: float = DEFAULTS["scale_factor"],
                 opa_init: float = DEFAULTS["opa_init"], color_dim: int = 3, scale_activation: str = "abs") -> "_lib.GsSeedOpts":
    return _lib.GsSeedOpts(int(stride), float(alpha_thresh), float(front_rel), float(scale_factor), float(opa_init),
                           SCALE_ACT[scale_activation], int(color_dim))


def seed_camera(camera) -> "_lib.GsSeedCamera":
    c = _lib.GsSeedCamera()
    c.rot, c.tran = pose_ctypes(camera)
    c.focal_x, c.focal_y = float(camera.focal_x), float(camera.focal_y)
    c.width, c.height = int(camera.width), int(camera.height)
    return c


def seed_camera_pp(camera) -> "_lib.GsSeedCameraPP":
    """``camera`` with its principal point's offset (``struct gs_seed_camera_pp``; (0, 0) for a centred camera)."""
    dx, dy = principal_point_offset(camera)
    return _lib.GsSeedCameraPP(seed_camera(camera), dx, dy)


def seed_classify(rng: torch.Tensor, rendered: Optional[Tuple[torch.Tensor, torch.Tensor]], opts):
    """The decision pass: -> (counts [2] int64 on the device = (selected, measured lattice pixels), workspace)."""
    require_hip(rng.device, "seeding")
    H, W = (int(v) for v in rng.shape)
    check_tensor("depth", rng, (H, W))
    d_ptr = a_ptr = None
    if rendered is not None:
        d_ptr, a_ptr = (check_tensor(n, t, (H, W)).data_ptr() for n, t in zip(("rendered depth", "rendered alpha"), rendered))
    ws = workspace(_lib.gs_seed_workspace_bytes(H, W), rng.device)
    counts = torch.zeros(2, dtype=torch.int64, device=rng.device)
    _lib.call("gs_seed_classify", rng.data_ptr(), d_ptr, a_ptr, H, W, C.byref(opts), counts.data_ptr(), ws.data_ptr(),
              ws.numel(), stream())
    return counts, ws


def seed_apply(image: torch.Tensor, rng: torch.Tensor, camera, opts, out: Sequence[torch.Tensor], offset: int,
               counts: torch.Tensor, ws: torch.Tensor, capacity: Optional[int] = None):
    """The write pass into rows [offset, offset + selected) of ``out`` = (pos, quat, scale, opa, rgb), arrays of ``capacity``
    rows (default: their length); writes nothing if they do not fit."""
    H, W = (int(v) for v in rng.shape)
    check_tensor("image", image, (H, W, 3))
    cap = int(out[0].shape[0]) if capacity is None else int(capacity)
    for name, t, tail in zip(("pos", "quat", "scale", "opa", "rgb"), out, ROW_SHAPES):
        check_tensor(name, t, rows_min=cap, tail=(int(opts.color_dim),) if tail is None else tail)
    cam = seed_camera(camera)
    if (cam.height, cam.width) != (H, W):
        raise RuntimeError(f"the maps are {H} x {W}, the camera is {cam.height} x {cam.width}")
    # the rays move with the principal point (gs_seed_apply_pp)
    pp = principal_point_offset(camera) != (0.0, 0.0)
    _lib.call("gs_seed_apply_pp" if pp else "gs_seed_apply", image.data_ptr(), rng.data_ptr(),
              C.byref(seed_camera_pp(camera) if pp else cam), C.byref(opts), *(t.data_ptr() for t in out), int(offset), cap,
              counts.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    # rows written through raw pointers into tensors the caller may already have rendered from (a set with spare capacity):
    # advance their version counters, which a renderer's scene pack is keyed on
    torch.autograd.graph.increment_version(tuple(out))


def seed_from_depth(image: torch.Tensor, depth: torch.Tensor, camera, *,
                    rendered: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, depth_kind: str = "range",
                    stride: int = DEFAULTS["stride"], alpha_thresh: float = DEFAULTS["alpha_thresh"],
                    front_rel: float = DEFAULTS["front_rel"], scale_factor: float = DEFAULTS["scale_factor"],
                    opa_init: float = DEFAULTS["opa_init"], color_dim: int = 3, scale_activation: str = "abs",
                    append_to: Optional[Sequence[torch.Tensor]] = None):
    """-> (pos, quat, scale, opa, rgb): the new Gaussians, or -- ``append_to`` = the five tensors of a Gaussian set -- that
    set with the new rows behind it (the old rows first, bit for bit).

    ``image`` [H,W,3] in [0,1] and ``depth`` [H,W] (<= 0, inf, NaN: no measurement) are the view's colour and depth frames,
    ``depth_kind`` "range" (distance from the camera centre, what the frame's depth map accumulates) or "z" (sensor z-depth:
    converted with ``gs_train.z_to_range``).  ``rendered`` = (depth_map, alpha_map) of the current model from ``camera``
    (``FrameRenderer.render_aux``); None: an empty model.  A measured pixel of the ``stride`` lattice is taken where
    alpha < ``alpha_thresh`` or range * alpha < (1 - ``front_rel``) * depth_map."""
    if depth_kind not in ("range", "z"):
        raise ValueError(f"depth_kind must be 'range' or 'z', got {depth_kind!r}")
    if depth_kind == "z":
        from gs_train import z_to_range

        depth = z_to_range(depth, camera).contiguous()
    opts = seed_options(stride, alpha_thresh, front_rel, scale_factor, opa_init, color_dim, scale_activation)
    if append_to is not None and int(append_to[4].shape[1]) != opts.color_dim:
        raise RuntimeError(f"append_to holds colour rows of {int(append_to[4].shape[1])}, color_dim is {opts.color_dim}")
    counts, ws = seed_classify(depth, rendered, opts)
    n_new = int(counts[0])  # the one host synchronisation
    n_old = int(append_to[0].shape[0]) if append_to is not None else 0
    if append_to is not None and n_new == 0:
        return tuple(append_to)
    dev = depth.device
    out = [torch.empty((n_old + n_new,) + (tail if tail is not None else (opts.color_dim,)), dtype=torch.float32, device=dev)
           for tail in ROW_SHAPES]
    if n_old:
        for o, t in zip(out, append_to):
            o[:n_old].copy_(t.detach())
    if n_new:
        seed_apply(image, depth, camera, opts, out, n_old, counts, ws)
    return tuple(out)
