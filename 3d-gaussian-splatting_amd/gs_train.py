"""Training step around the frame path: image loss, fused Adam, the reference's LR schedule.

Mirrors ``Trainer.__init__`` / ``Trainer.train_step`` of the reference (train.py:16-67, 84-200) for the
part that runs every iteration:

    forward -> loss = (1-w) L1 + w (1-SSIM) -> backward -> [all-reduce] -> Adam step -> LR update

with three differences that matter on MI355X:
  * the loss and its gradient are one streaming HIP kernel + a one-block reduction (``gs_loss_l1_ssim``) instead of ~40 torch kernels
    over five padded copies of the image (torchmetrics SSIM + autograd);
  * Adam is ONE launch over the flat parameter bucket (``gs_adam_step``), which also accumulates the
    densification statistic ``accum_max_grad`` of train.py:145-154 while it reads the gradient;
  * nothing in the step synchronises with the host: the reference calls ``.item()`` three times per
    iteration (train.py:119-121); here the losses stay on the device until somebody reads them.
Densification (``Trainer(..., densify=True)``: ``gs_densify.adaptive_control`` / ``reset_opa`` on the reference's
schedule) is SURVEY 8f-2; data loading and the viewer stay out of scope (8f-3, 8f-4).
"""
from __future__ import annotations

import ctypes as C
import os
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace
from gs_dp import ORDER, FlatGaussianParams, ViewParallelGradStat
from gs_frame import CONTRIB_W_MIN, Contributions, FrameRenderer
from gs_geometry import RayBasis, TileGrid, pose64, posed, principal_point_offset

GROUPS = ("opa", "rgb", "pos", "scale", "quat")  # the reference's param-group order (train.py:59-65)


@dataclass
class TrainOptions:
    """Defaults of the reference's argparse (train.py:297-347) for the options the step uses."""
    lr: float = 0.003
    lr_factor_for_scale: float = 1.0
    lr_factor_for_rgb: float = 10.0
    lr_factor_for_opa: float = 10.0
    lr_factor_for_quat: float = 1.0
    lr_decay: str = "exp"  # "none" | "official" | "exp"
    n_iters: int = 7001
    n_iters_warmup: int = 300
    ssim_weight: float = 0.1
    scale_reg: float = 0.0  # train.py:108-109: + scale_reg * mean |scale|
    opa_reg: float = 0.0    # train.py:110-112: + opa_reg * mean sigma(opa) (1 - sigma(opa))
    grad_accum_method: str = "max"  # "max" | "mean"
    betas: tuple = (0.9, 0.99)
    eps: float = 1e-8
    # densification (train.py:302, 321-324, 340-347); off unless Trainer(..., densify=True)
    n_adaptive_control: int = 100
    adaptive_control_start_iter: int = 600  # the literal `i_iter > 600` of train.py:88-90
    adaptive_control_end_iter: int = 1000000000
    grad_accum_iters: int = 50
    n_opa_reset: int = 10000000
    reset_interval: int = 500
    split_thresh: float = 0.05
    delete_thresh: float = 1.5
    grad_thresh: float = 0.0002
    grad_aggregation: str = "max"
    use_clone: int = 0
    use_split: int = 1
    clone_dt: float = 0.01
    # depth supervision (Trainer(..., depths=...)): + depth_weight * mean over the view's measured pixels of |r|, with
    # r = D - A z ("residual": no division, defined everywhere) or D / A - z ("expected": where A >= depth_alpha_min);
    # D, A the frame's depth / alpha maps, z the measured range (gs_loss_depth, include/gs_abi.h).  0: rgb only.
    depth_weight: float = 0.0
    depth_mode: str = "residual"  # "residual" | "expected"
    depth_alpha_min: float = 0.5


def lr_lambdas(opt: TrainOptions) -> List[Callable[[int], float]]:
    """The five per-group multipliers of train.py:29-58, in GROUPS order."""
    w = opt.n_iters_warmup
    warm = lambda i: i / w  # noqa: E731  (i <= warmup)
    if opt.lr_decay == "none":
        f = lambda i: warm(i) if i <= w else 0.2 ** ((i - w) // 2000)  # noqa: E731
        return [f] * 5
    gamma = 0.01 ** (1 / (opt.n_iters - w))
    decay = lambda i: warm(i) if i <= w else gamma ** (i - w)  # noqa: E731
    flat = lambda i: warm(i) if i <= w else 1  # noqa: E731
    if opt.lr_decay == "official":
        return [decay, flat, decay, flat, flat]
    if opt.lr_decay != "exp":
        raise ValueError(f"lr_decay must be none|official|exp, got {opt.lr_decay!r}")
    return [decay] * 5


def base_lrs(opt: TrainOptions) -> List[float]:
    """train.py:20-25, in GROUPS order."""
    return [opt.lr * opt.lr_factor_for_opa, opt.lr * opt.lr_factor_for_rgb, opt.lr * 1,
            opt.lr * opt.lr_factor_for_scale, opt.lr * opt.lr_factor_for_quat]


class FusedAdam:
    """``torch.optim.Adam`` over a FlatGaussianParams buffer: ONE HIP launch per step on a single GPU, one launch per
    exchange slice (five element ranges each, ``gs_adam_step_multi``) under view parallelism.

    With ``flat.exchange == "reduce_scatter"`` the optimizer is SHARDED: this rank keeps the moments of its 1/world shard
    of every slice range only (densely packed, slice by slice) and updates those shards only (gs_dp.py); otherwise every
    rank updates everything and the moments mirror the flat buffer."""

    def __init__(self, flat: FlatGaussianParams, lrs: Sequence[float], betas=(0.9, 0.99), eps: float = 1e-8,
                 grad_stat: Optional[str] = None):
        require_hip(flat.flat_param.device, "FusedAdam")
        self.flat = flat
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.sharded = flat.exchange == "reduce_scatter"
        dev = flat.flat_param.device
        size = self._build_units()
        self.exp_avg = torch.zeros(size, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step_count = 0
        # buffer storage order (gs_dp.ORDER) -> group boundaries; lrs arrive in the reference's GROUPS order
        ends = list(flat.group_ends)
        self._ends = (C.c_int64 * len(ends))(*ends)
        self._lr = (C.c_float * len(ends))()
        self.set_lrs(lrs)
        self._stat_range = flat.offsets["pos"]
        self.stat_mode = {None: 0, "max": 1, "mean": 2}[grad_stat]
        self.accum_grad = torch.zeros_like(flat.params[0]) if self.stat_mode else None  # train.py:80-82
        self.skip_flag = None  # device address of a 64-bit counter: non-zero => the step is skipped (gs_abi.h)

    def _build_units(self) -> int:
        """Per exchange slice: the (up to five) element ranges this rank updates and where their moments start -> size of
        the moment arrays."""
        flat = self.flat
        self._units = []
        off = 0
        for k in range(flat.n_slices):
            own = [r for r in flat.owned(flat.slice_ranges(k)) if r[1] > r[0]]
            offs = []
            for lo, hi in own:
                offs.append(off if self.sharded else lo)  # replicated: the moments mirror the flat buffer
                off += hi - lo
            n_r = len(own)
            self._units.append((n_r, (C.c_int64 * n_r)(*[r[0] for r in own]), (C.c_int64 * n_r)(*[r[1] for r in own]),
                                (C.c_int64 * n_r)(*offs)))
        return off if self.sharded else flat.flat_param.numel()

    def moment_rows(self, name: str):
        """(exp_avg, exp_avg_sq) of parameter tensor ``name`` as views shaped like it -- a replicated optimizer only, whose
        moments mirror the flat buffer (a sharded one keeps 1 / world of them, packed by slice)."""
        if self.sharded:
            raise RuntimeError("a sharded optimizer's moments are not addressable by row")
        lo, hi = self.flat.offsets[name]
        shape = self.flat.params[("pos", "quat", "scale", "opa", "rgb").index(name)].shape
        return self.exp_avg[lo:hi].view(shape), self.exp_avg_sq[lo:hi].view(shape)

    def reslice(self):
        """After ``flat.set_slices``: a replicated optimizer's moments mirror the flat buffer, so only the unit tables
        change; a sharded one packs its moments by slice and cannot follow."""
        if self.sharded:
            raise RuntimeError("a sharded optimizer cannot be re-sliced (its moments are packed slice by slice)")
        self._build_units()

    @property
    def state_bytes(self) -> int:
        """Optimizer state this rank keeps (both moments)."""
        return self.exp_avg.numel() * 8

    def set_lrs(self, lrs: Sequence[float]):
        by_group = dict(zip(GROUPS, lrs))
        for i, k in enumerate(ORDER):
            self._lr[i] = float(by_group[k])

    def clear_grad_stat(self):
        if self.accum_grad is not None:
            self.accum_grad.zero_()

    def step(self, advance: bool = True):
        """One Adam step over everything this rank owns (the step counter advances once per optimizer step).  Note: a
        step the device skips because its frame overflowed (``skip_flag``) still counts for the bias corrections --
        the host cannot know without synchronising."""
        if advance:
            self.step_count += 1
        if self.sharded:
            for k in range(len(self._units)):
                self.step_slice(k, advance=False)
            return
        f = self.flat
        b, e = self._stat_range
        n = f.flat_param.numel()
        _lib.call("gs_adam_step_sharded",
                  f.flat_param.data_ptr(), f.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n, 0, n,
                  0, len(ORDER), self._ends, self._lr, self.betas[0], self.betas[1], self.eps, self.step_count,
                  self.accum_grad.data_ptr() if self.accum_grad is not None else None, b, e, self.stat_mode, self.skip_flag,
                  stream())
        # the kernel wrote the flat buffer through a raw pointer: advance its version counter (shared by all its views, the
        # five parameter tensors among them), which a renderer's scene pack is keyed on
        torch.autograd.graph.increment_version(f.flat_param)

    def fused_descriptor(self, advance: bool = True):
        """The ``gs_adam_fused`` argument of ``FrameRenderer.backward_adam`` for ONE optimizer step over everything
        (replicated optimizer: the moments mirror the flat buffer).  Advances the step counter like ``step``."""
        if self.sharded:
            raise RuntimeError("the fused backward + Adam step needs a replicated optimizer")
        if advance:
            self.step_count += 1
        f = self.flat
        d = _lib.GsAdamFused()
        lr_of = dict(zip(ORDER, self._lr))
        for i, name in enumerate(("pos", "quat", "scale", "opa", "rgb")):
            off = f.offsets[name][0] * 4
            d.exp_avg[i] = self.exp_avg.data_ptr() + off
            d.exp_avg_sq[i] = self.exp_avg_sq.data_ptr() + off
            d.lr[i] = lr_of[name]
        d.beta1, d.beta2, d.eps, d.step = self.betas[0], self.betas[1], self.eps, self.step_count
        d.grad_stat = self.accum_grad.data_ptr() if self.accum_grad is not None else None
        d.stat_mode = self.stat_mode
        d.skip_if_nonzero = self.skip_flag
        return d

    def step_slice(self, k: int, advance: bool = False, grad_scale: float = 1.0):
        """The same step for exchange slice ``k`` only (pass ``advance=True`` for the first slice of a step).
        ``grad_scale``: the gradient enters as grad * grad_scale (1 / world after a SUM exchange: gs_dp.py)."""
        if advance:
            self.step_count += 1
        n_r, lo, hi, off = self._units[k]
        if n_r == 0:
            return
        f = self.flat
        b, e = self._stat_range
        _lib.call("gs_adam_step_multi",
                  f.flat_param.data_ptr(), f.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                  f.flat_param.numel(), n_r, lo, hi, off, len(ORDER), self._ends, self._lr, self.betas[0], self.betas[1],
                  self.eps, self.step_count, self.accum_grad.data_ptr() if self.accum_grad is not None else None, b, e,
                  self.stat_mode, self.skip_flag, float(grad_scale), stream())
        torch.autograd.graph.increment_version(f.flat_param)  # (as in `step`)


class _MapLoss:
    """What the loss objects share: the refusal of a non-HIP device and the workspace."""

    def _setup(self, height: int, width: int, device, workspace_bytes):
        self.H, self.W = int(height), int(width)
        self.device = require_hip(device, type(self).__name__)
        self._ws = workspace(workspace_bytes(self.H, self.W), self.device)

    def _new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)


class ImageLoss(_MapLoss):
    """``(1-w) * L1 + w * (1 - SSIM)`` and its gradient w.r.t. the rendered image (train.py:99-107)."""

    def __init__(self, height: int, width: int, ssim_weight: float = 0.1, device="cuda"):
        self.w = float(ssim_weight)
        self._setup(height, width, device, _lib.gs_loss_workspace_bytes)
        self.grad = self._new(self.H, self.W, 3)
        self.values = torch.zeros(3, dtype=torch.float32, device=self.device)  # (loss, l1, ssim), stays on device

    def __call__(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        for name, t in (("pred", pred), ("target", target)):
            check_tensor(name, t, (self.H, self.W, 3))
        _lib.call("gs_loss_l1_ssim", pred.data_ptr(), target.data_ptr(), self.H, self.W, self.w, self.grad.data_ptr(),
                  self.values.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream())
        return self.grad


def weight_sums(weight: torch.Tensor) -> Tuple[float, float]:
    """(sum of a weight map [H,W], its sum over the SSIM interior -- rows 5 .. H-6, columns 5 .. W-6; 0 when H <= 10 or
    W <= 10), in double: the two host arguments of ``gs_loss_l1_ssim_weighted``.  One host read; a caller takes them once
    per view."""
    h, w = weight.shape
    total = weight.sum(dtype=torch.float64)
    inner = weight[5:h - 5, 5:w - 5].sum(dtype=torch.float64) if h > 10 and w > 10 else torch.zeros_like(total)
    total, inner = torch.stack([total, inner]).tolist()
    return float(total), float(inner)


class WeightedImageLoss(_MapLoss):
    """``ImageLoss`` with a per-pixel weight map [H,W] (finite, >= 0; gs_loss_l1_ssim_weighted, include/gs_abi.h): both terms
    become weighted means.  The call takes the map and its two sums (``weight_sums``: the caller computes them once per view
    and validates the map then -- the kernel checks neither); an all-ones map with sums H W and (H-10)(W-10) gives
    ``ImageLoss``'s gradient and values bit for bit.  Same ``grad`` / ``values`` members as ``ImageLoss``."""

    def __init__(self, height: int, width: int, ssim_weight: float = 0.1, device="cuda"):
        self.w = float(ssim_weight)
        self._setup(height, width, device, _lib.gs_loss_workspace_bytes)
        self.grad = self._new(self.H, self.W, 3)
        self.values = torch.zeros(3, dtype=torch.float32, device=self.device)  # (loss, l1, ssim), stays on device

    def __call__(self, pred: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, weight_sum: float,
                 weight_sum_interior: float) -> torch.Tensor:
        for name, t in (("pred", pred), ("target", target)):
            check_tensor(name, t, (self.H, self.W, 3))
        check_tensor("weight", weight, (self.H, self.W))
        _lib.call("gs_loss_l1_ssim_weighted", pred.data_ptr(), target.data_ptr(), weight.data_ptr(), self.H, self.W, self.w,
                  float(weight_sum), float(weight_sum_interior), self.grad.data_ptr(), self.values.data_ptr(),
                  self._ws.data_ptr(), self._ws.numel(), stream())
        return self.grad


class DepthLoss(_MapLoss):
    """``scale * sum |r|`` over the measured pixels of a range map and its gradients w.r.t. the depth / alpha maps of an aux
    frame (gs_loss_depth, include/gs_abi.h): ``mode`` "residual" (r = D - A z) or "expected" (r = D / A - z where
    A >= ``alpha_min``).  Owns the workspace and the two gradient maps; ``values`` = (loss, pixels that counted)."""

    MODES = {"residual": 0, "expected": 1}

    def __init__(self, height: int, width: int, mode: str = "residual", alpha_min: float = 0.5, device="cuda"):
        if mode not in self.MODES:
            raise ValueError(f"depth mode must be 'residual' or 'expected', got {mode!r}")
        self.mode, self.alpha_min = self.MODES[mode], float(alpha_min)
        self._setup(height, width, device, _lib.gs_loss_depth_workspace_bytes)
        self.grad_depth, self.grad_alpha = self._new(self.H, self.W), self._new(self.H, self.W)
        self.values = torch.zeros(2, dtype=torch.float32, device=self.device)  # stays on the device

    def __call__(self, depth: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, scale: float):
        """``target``: [H,W] range from the camera centre (<= 0, inf, NaN: no measurement); ``scale``: weight / number of
        measured pixels.  Returns (grad_depth, grad_alpha)."""
        for name, t in (("depth", depth), ("alpha", alpha), ("target", target)):
            check_tensor(name, t, (self.H, self.W))
        _lib.call("gs_loss_depth", depth.data_ptr(), alpha.data_ptr(), target.data_ptr(), self.H, self.W, self.mode,
                  self.alpha_min, float(scale), self.grad_depth.data_ptr(), self.grad_alpha.data_ptr(), self.values.data_ptr(),
                  self._ws.data_ptr(), self._ws.numel(), stream())
        return self.grad_depth, self.grad_alpha


class _TrackMaps(_MapLoss):
    """What the two tracking losses share: the three gradient maps, ``values``, and the check of a call's arguments."""

    def _setup(self, height: int, width: int, device, workspace_bytes, n_values: int):
        super()._setup(height, width, device, workspace_bytes)
        self.grad_image = self._new(self.H, self.W, 3)
        self.grad_depth, self.grad_alpha = self._new(self.H, self.W), self._new(self.H, self.W)
        self.values = torch.zeros(n_values, dtype=torch.float32, device=self.device)  # stays on the device

    def _checked(self, image, depth, alpha, target_image, target_range, values):
        """The five input maps checked (``target_range`` may be None) -> the checked destination of the values."""
        maps = [("image", image, (3,)), ("depth", depth, ()), ("alpha", alpha, ()), ("target_image", target_image, (3,))]
        if target_range is not None:
            maps.append(("target_range", target_range, ()))
        for name, t, c in maps:
            check_tensor(name, t, (self.H, self.W) + c)
        if values is None:
            return self.values
        if check_tensor("values", values).numel() != self.values.numel():
            raise RuntimeError(f"values must hold {self.values.numel()} floats, got {values.numel()}")
        return values


class TrackLoss(_TrackMaps):
    """The loss of camera tracking against a frozen map and its gradients w.r.t. the image, depth and alpha maps of an aux
    frame (gs_loss_track, include/gs_abi.h): ``scale * (color_weight * sum |I - T| + depth_weight * sum |D / A - z|)`` over
    the pixels the map covers (A >= ``alpha_min``), the depth term on those that are measured and pass ``depth_gate``
    (<= 0: off).  Owns the workspace and the three gradient maps; ``values`` = (loss, colour term, depth term, pixels that
    counted for depth) unless the call names another destination."""

    def __init__(self, height: int, width: int, alpha_min: float = 0.5, color_weight: float = 1.0, depth_weight: float = 1.0,
                 depth_gate: float = 0.0, device="cuda"):
        self.alpha_min = float(alpha_min)
        self.color_weight, self.depth_weight, self.depth_gate = float(color_weight), float(depth_weight), float(depth_gate)
        self._setup(height, width, device, _lib.gs_loss_track_workspace_bytes, 4)

    def __call__(self, image: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, target_image: torch.Tensor,
                 target_range: Optional[torch.Tensor], scale: float, values: Optional[torch.Tensor] = None):
        """``target_range``: [H,W] range from the camera centre (<= 0, inf, NaN: no measurement) or None (RGB only);
        ``values``: four contiguous float32 on the device to receive the values in place of ``self.values``.  Returns
        (grad_image, grad_depth, grad_alpha)."""
        values = self._checked(image, depth, alpha, target_image, target_range, values)
        _lib.call("gs_loss_track", image.data_ptr(), depth.data_ptr(), alpha.data_ptr(), target_image.data_ptr(),
                  target_range.data_ptr() if target_range is not None else None, self.H, self.W, self.alpha_min,
                  self.color_weight, self.depth_weight, self.depth_gate, float(scale), self.grad_image.data_ptr(),
                  self.grad_depth.data_ptr(), self.grad_alpha.data_ptr(), values.data_ptr(), self._ws.data_ptr(),
                  self._ws.numel(), stream())
        return self.grad_image, self.grad_depth, self.grad_alpha


class GatedTrackLoss(_TrackMaps):
    """``TrackLoss`` with each term gated at a multiple of the frame's own median residual (gs_loss_track_gated,
    include/gs_abi.h): depth counts where |D / A - z| <= max(``depth_gate_k`` x its lower median over the covered, measured
    pixels, ``depth_gate_floor``), colour where sum_c |I_c - T_c| <= max(``color_gate_k`` x its lower median over the covered
    pixels, ``color_gate_floor``); a k <= 0 switches that term's gate off; with ``couple`` a pixel that fails the depth gate
    loses its colour term too.  The medians are selected on the device: no host synchronisation.  The call shape of
    ``TrackLoss``; ``values`` = (loss, colour term, depth term, depth pixels that counted, colour pixels that counted, m_d,
    m_c, n_d).  ``keep_residuals=True`` exposes the two residual maps the kernels store (``resid_depth`` = |D / A - z|,
    ``resid_color`` = sum_c |I_c - T_c| at the pixels of their sets, NaN elsewhere); otherwise they live in the workspace."""

    def __init__(self, height: int, width: int, alpha_min: float = 0.5, color_weight: float = 1.0, depth_weight: float = 1.0,
                 depth_gate_k: float = 0.0, color_gate_k: float = 0.0, depth_gate_floor: float = 0.0,
                 color_gate_floor: float = 0.0, couple: bool = True, device="cuda", keep_residuals: bool = False):
        self.alpha_min = float(alpha_min)
        self.color_weight, self.depth_weight = float(color_weight), float(depth_weight)
        self.depth_gate_k, self.color_gate_k = float(depth_gate_k), float(color_gate_k)
        self.depth_gate_floor, self.color_gate_floor = float(depth_gate_floor), float(color_gate_floor)
        self.couple = bool(couple)
        self._setup(height, width, device, _lib.gs_loss_track_gated_workspace_bytes, 8)
        self.resid_depth = self._new(self.H, self.W) if keep_residuals else None
        self.resid_color = self._new(self.H, self.W) if keep_residuals else None

    def __call__(self, image: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, target_image: torch.Tensor,
                 target_range: Optional[torch.Tensor], scale: float, values: Optional[torch.Tensor] = None):
        """As ``TrackLoss.__call__``; ``values``: eight contiguous float32 on the device to receive the values in place of
        ``self.values``.  Returns (grad_image, grad_depth, grad_alpha)."""
        values = self._checked(image, depth, alpha, target_image, target_range, values)
        _lib.call("gs_loss_track_gated", image.data_ptr(), depth.data_ptr(), alpha.data_ptr(), target_image.data_ptr(),
                  target_range.data_ptr() if target_range is not None else None, self.H, self.W, self.alpha_min,
                  self.color_weight, self.depth_weight, self.depth_gate_k, self.color_gate_k, self.depth_gate_floor,
                  self.color_gate_floor, int(self.couple), float(scale), self.grad_image.data_ptr(), self.grad_depth.data_ptr(),
                  self.grad_alpha.data_ptr(), values.data_ptr(),
                  self.resid_depth.data_ptr() if self.resid_depth is not None else None,
                  self.resid_color.data_ptr() if self.resid_color is not None else None, self._ws.data_ptr(), self._ws.numel(),
                  stream())
        return self.grad_image, self.grad_depth, self.grad_alpha


class GateMask(_MapLoss):
    """The median gate of ``GatedTrackLoss`` as the mapping inputs of a keyframe (gs_track_gate_mask, include/gs_abi.h): from
    the frozen map rendered at the frame's pose with its aux maps and the incoming frame, ``range`` -- the range map with the
    measurements the depth gate rejects written as 0, "no measurement" -- and ``weight`` -- 0 where the map covers the pixel
    and its colour term does not count (the coupling included), else 1.  The tracker's exact sets, medians and thresholds; a
    pixel the map does not cover keeps its range and has weight 1.  The call shape of ``GatedTrackLoss`` without ``scale``;
    ``values`` = (measured pixels, range pixels kept, range pixels removed, sum of weight, its sum over the SSIM interior,
    m_d, m_c, n_d), on the device.  Owns the workspace, ``range``, ``weight`` and ``values``; a call without a range map
    leaves ``range`` untouched."""

    def __init__(self, height: int, width: int, alpha_min: float = 0.5, depth_gate_k: float = 0.0, color_gate_k: float = 0.0,
                 depth_gate_floor: float = 0.0, color_gate_floor: float = 0.0, couple: bool = True, device="cuda"):
        self.alpha_min = float(alpha_min)
        self.depth_gate_k, self.color_gate_k = float(depth_gate_k), float(color_gate_k)
        self.depth_gate_floor, self.color_gate_floor = float(depth_gate_floor), float(color_gate_floor)
        self.couple = bool(couple)
        self._setup(height, width, device, _lib.gs_track_gate_mask_workspace_bytes)
        self.range, self.weight = self._new(self.H, self.W), self._new(self.H, self.W)
        self.values = torch.zeros(8, dtype=torch.float32, device=self.device)  # stays on the device

    @classmethod
    def from_track_options(cls, height: int, width: int, opt, device="cuda") -> "GateMask":
        """The gate a ``gs_track.TrackOptions`` describes (alpha_min, the two k, the two floors, gate_couple)."""
        return cls(height, width, opt.alpha_min, opt.depth_gate_k, opt.color_gate_k, opt.depth_gate_floor,
                   opt.color_gate_floor, opt.gate_couple, device)

    def __call__(self, image: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, target_image: torch.Tensor,
                 target_range: Optional[torch.Tensor]):
        """``target_range``: [H,W] range from the camera centre (<= 0, inf, NaN: no measurement) or None (an RGB-only gate).
        Returns (range or None, weight)."""
        maps = [("image", image, (3,)), ("depth", depth, ()), ("alpha", alpha, ()), ("target_image", target_image, (3,))]
        if target_range is not None:
            maps.append(("target_range", target_range, ()))
        for name, t, c in maps:
            check_tensor(name, t, (self.H, self.W) + c)
        _lib.call("gs_track_gate_mask", image.data_ptr(), depth.data_ptr(), alpha.data_ptr(), target_image.data_ptr(),
                  target_range.data_ptr() if target_range is not None else None, self.H, self.W, self.alpha_min,
                  self.depth_gate_k, self.color_gate_k, self.depth_gate_floor, self.color_gate_floor, int(self.couple),
                  self.range.data_ptr() if target_range is not None else None, self.weight.data_ptr(), self.values.data_ptr(),
                  None, None, self._ws.data_ptr(), self._ws.numel(), stream())
        return (self.range if target_range is not None else None), self.weight


def z_to_range(z: torch.Tensor, camera) -> torch.Tensor:
    """Sensor z-depth [H,W] (distance along the optical axis) -> range from the camera centre, what the aux depth map
    measures (d_i = |p_c|): range = z |ray| / ray_z with the renderer's own per-pixel rays (gs_geometry.RayBasis: pixel
    centres of the padded image, cropped like the image), so the conversion and the rendered map agree on where a pixel
    looks.  Pixels without a measurement (<= 0, inf, NaN) stay what they are."""
    grid = TileGrid(int(camera.width), int(camera.height), float(camera.focal_x), float(camera.focal_y))
    rays = RayBasis.from_camera(camera.rot, camera.tran, grid.padded_height, grid.padded_width, grid.focal_x, grid.focal_y,
                                pp_offset=principal_point_offset(camera))  # (the rays of the camera's own principal point)
    top, left = grid.crop_offsets()
    px = (np.arange(grid.width, dtype=np.float64) + left)[None, :, None]
    py = (np.arange(grid.height, dtype=np.float64) + top)[:, None, None]
    d = (rays.lefttop.astype(np.float64) - rays.rays_o.astype(np.float64))[None, None, :] \
        + px * rays.dx.astype(np.float64)[None, None, :] + py * rays.dy.astype(np.float64)[None, None, :]
    axis = np.asarray(camera.rot, np.float64).reshape(3, 3)[2]  # the optical axis in world coordinates
    factor = np.linalg.norm(d, axis=2) / (d @ axis)
    return (z.to(torch.float64) * torch.from_numpy(factor).to(z.device)).to(torch.float32)


@dataclass
class _Carry:
    """What ``Trainer._bind`` takes over from the optimizer it replaces when the Gaussian set is EDITED rather than replaced:
    the step count, and ``fill(flat, optimizer)``, which writes the rows that travel into the new (zeroed) buffers."""
    step_count: int
    fill: Callable


class Trainer:
    """One view per step on this rank; gradients are averaged over ranks when torch.distributed is up.

    NOTE for callers that read gradients: with ``fuse_adam`` active (the default on one rank, rgb or SH colours) the
    optimizer step runs inside the backward's last kernel and ``flat.grads`` is NOT written -- it holds whatever an
    earlier, unfused step left there.  Pass ``fuse_adam=False`` to get the gradients of every step."""

    def __init__(self, params: Sequence[torch.Tensor], cameras, targets: Sequence[torch.Tensor],
                 opt: Optional[TrainOptions] = None, world_size: int = 1, max_pairs: int = 1 << 20,
                 scale_activation: str = "abs", densify: bool = False, generator: Optional[torch.Generator] = None,
                 per_view_stat: Optional[bool] = None, exchange: str = "all_reduce", n_slices: Optional[int] = None,
                 bwd_rows: Optional[bool] = None, fuse_adam: Optional[bool] = None,
                 depths: Optional[Sequence[Optional[torch.Tensor]]] = None, depth_kind: str = "range",
                 weights: Optional[Sequence[Optional[torch.Tensor]]] = None, densify_carry: bool = False,
                 exposures: Optional[dict] = None):
        self.opt = opt or TrainOptions()
        # `weights`: a list parallel to `targets`, each entry a per-pixel weight map [H,W] float32 (finite, >= 0) for the
        # view's colour loss or None.  A view with a map takes the weighted loss (WeightedImageLoss) where the step calls its
        # image loss; a view without one issues exactly the calls it issues without `weights`.  Validated once per view,
        # its two sums taken once, in double (_view_weight).  `test` / `psnr` stay unweighted.
        self.weights, self._weight_sums = None, None
        if weights is not None:
            if len(weights) != len(targets):
                raise ValueError("weights must be a list parallel to targets (None for a view without a weight map)")
            views = [self._view_weight(cam_, w_, params[0].device) for cam_, w_ in zip(cameras, weights)]
            self.weights, self._weight_sums = [v[0] for v in views], [v[1] for v in views]
        self._weighted_loss = {}
        # `depths`: a list parallel to `targets`, each entry a measured depth map [H,W] float32 or None (a view without one).
        # `depth_kind`: "range" = distance from the camera centre, what the frame's depth map accumulates; "z" = sensor
        # z-depth, converted once here with the renderer's own rays (z_to_range).  Pixels <= 0, inf or NaN carry no
        # measurement.  With opt.depth_weight > 0 a view that has a map is rendered with its depth / alpha maps and
        # trained on colour AND depth (train_step); every other step issues exactly the calls it issues without `depths`.
        if depth_kind not in ("range", "z"):
            raise ValueError(f"depth_kind must be 'range' or 'z', got {depth_kind!r}")
        if self.opt.depth_mode not in DepthLoss.MODES:
            raise ValueError(f"depth_mode must be 'residual' or 'expected', got {self.opt.depth_mode!r}")
        self.depths, self._depth_inv_n = None, None
        self._depth_kind, self._depth_device = depth_kind, params[0].device
        if depths is not None:
            if len(depths) != len(targets):
                raise ValueError("depths must be a list parallel to targets (None for a view without a depth map)")
            self.depths, self._depth_inv_n = [], []
            for cam_, d in zip(cameras, depths):
                d, inv_n = self._view_depth(cam_, d)
                self.depths.append(d)
                self._depth_inv_n.append(inv_n)
        self._depth_loss = {}
        self.depth_loss = None  # the DepthLoss of the last depth-supervised step (.values: loss, pixels that counted)
        # `fuse_adam`: apply the Adam step inside the backward's last kernel (FrameRenderer.backward_adam: no gradient buffer is
        # written, bit-identical parameters) where the step allows it -- one rank, no regulariser that edits the
        # gradient, the densification statistic fused into the optimizer.  None: on (GS_TRAIN_FUSE_ADAM=0 turns it off for
        # A/B runs of bench.py); False: never (a caller that reads flat.grads behind a step).  Same-box A/B, round 5
        # (profiles/r05_r_*): 775 against 745 it/s on the moving 2.4 M-Gaussian scene, 933 against 894 fixed, 1786 against
        # 1738 at 376 k -- one 208 us kernel where the projection backward (113 us) and gs_adam_step (150 us) ran.  (The
        # first version -- every thread its own 14 parameters, 84 four-byte accesses at a 12-byte stride -- was 15 % SLOWER
        # than the two kernels, r05_q; the float4 walk through an LDS hand-over is what made it pay.)
        if fuse_adam is None:
            fuse_adam = os.environ.get("GS_TRAIN_FUSE_ADAM", "") != "0"
        self.fuse_adam = bool(fuse_adam)
        self.world_size = int(world_size)
        self.n_slices = n_slices  # exchange slices of the Gaussian array (gs_dp.py; None: by scene size)
        if exchange == "reduce_scatter" and self.world_size > 1:
            import torch.distributed as dist

            if not dist.is_initialized():
                # every rank would keep and update its own 1/world of the optimizer state while nobody exchanges
                # anything: (world - 1)/world of the parameters would silently never train
                raise RuntimeError("exchange='reduce_scatter' with world_size > 1 needs an initialised process group")
        # gradient exchange under view parallelism (gs_dp.py): "all_reduce" + replicated Adam, or "reduce_scatter" +
        # sharded Adam + all-gather of the parameters
        self.exchange = exchange
        # `densify_carry`: every adaptive_control of the schedule EDITS the running fit instead of restarting it -- the rows that
        # survive keep their Adam moments, new rows (and split ones) start from zero, the step count goes on -- and an opacity
        # reset zeroes the opacity moments (what the original 3DGS optimizer does; the reference restarts Adam, and so does the
        # default).  One rank with a replicated optimizer only: refused here, not at the first control iteration.
        self.densify_carry = bool(densify_carry)
        if self.densify_carry:
            self._refuse_carry("Trainer(densify_carry=True)", stat=False)
        # densification statistic: fused into the Adam launch on one GPU; with several ranks it must be taken from
        # each rank's own gradient before the all-reduce (gs_dp.ViewParallelGradStat).  `per_view_stat=True` forces
        # that path on a single rank too (it then gives bit-identical results; used by the tests).
        self.per_view_stat = (self.world_size > 1) if per_view_stat is None else bool(per_view_stat)
        self.scale_activation = scale_activation
        self.densify, self.generator = bool(densify), generator
        self.cameras, self.targets = list(cameras), list(targets)
        dev = params[0].device
        # "async": in steady state the pair capacity is checked from a pinned-memory copy one frame late -- no host
        # synchronisation in the training loop (the reference synchronises >= 8 times per forward).  The FIRST frame
        # of every view on every Gaussian set (start of training, after each densification) is checked synchronously
        # and redone in a larger workspace if it did not fit, so a step is never taken on an empty frame because the
        # capacity was simply unknown; after that a view's pair count only drifts, and the workspace grows ahead of
        # it (25 % head room).  Should a frame overflow all the same, `renderer.overflowed_frames` counts it and
        # train_step warns once the late counters arrive.
        # `bwd_rows`: which kernel composites the rgb backward (FrameRenderer; None: by the scene's share of saturated
        # buckets, asked for ONCE per Gaussian set -- behind its first step -- so that a run takes the same kernels, the
        # same bits, every time).
        self.renderer = FrameRenderer(dev, max_pairs=max_pairs, training=True, scale_activation=scale_activation,
                                      auto_grow="async", bwd_rows=bwd_rows)
        self._backward_choice_due = True
        self._views_checked = set()
        self._overflow_warned = 0
        self._lambdas, self._base = lr_lambdas(self.opt), base_lrs(self.opt)
        self._loss = {}
        self._free = {}  # camera id -> _FreePose: gs_track.FreePose: the views whose pose is refined with the map (free_pose)
        # `exposures`: {camera id: (gain [3], bias [3])}, the affine exposure of the views that have one (gs_exposure.Exposure:
        # six numbers in device memory).  Such a view's colour loss -- plain or weighted -- is taken on the compensated render,
        # and the exposure's backward scales the gradient map before it travels through whichever backward the step takes;
        # fixed unless `free_exposure` frees it.  A view without one issues exactly the calls it issues without `exposures`,
        # and no Exposure object exists for it.  `test` and every evaluation render stay uncompensated.
        self._exposure = {}
        for cid, (gain, bias) in (exposures or {}).items():
            if not 0 <= int(cid) < len(self.cameras):
                raise IndexError(f"exposures names view {cid}: no such view")
            self._exposure[int(cid)] = self._view_exposure(self.cameras[int(cid)], (gain, bias), dev)
        self._bind(params, 0)

    def _bind(self, params: Sequence[torch.Tensor], i_iter: int, carry: Optional[_Carry] = None):
        """(Re)creates the flat bucket and the optimizer for a (new) Gaussian set: train.py:59-67 / :169-179 --
        the reference also starts a fresh torch.optim.Adam after every adaptive_control.  ``carry`` (an edit of the set:
        ``prune``, ``seed_from_view(carry_state=True)``): the new optimizer keeps the old step count and ``carry.fill`` writes
        the carried rows of the moments and the statistic into its zeroed buffers (pad rows stay zero); everything else is
        the rebind it always was."""
        force = getattr(getattr(self, "flat", None), "force_collective", False)
        self.flat = FlatGaussianParams(params, world_size=self.world_size, exchange=self.exchange,
                                       force_collective=force, n_slices=self.n_slices)
        self.flat.mean_in_optimizer = True  # the exchange sums, step_slice applies 1 / world (gs_dp.py)
        self.renderer.forward_abandon()  # a frame projected ahead belonged to the old Gaussian set
        split_stat = self.densify and self.per_view_stat
        self.optimizer = FusedAdam(self.flat, [b * f(i_iter) for b, f in zip(self._base, self._lambdas)],
                                   betas=self.opt.betas, eps=self.opt.eps,
                                   grad_stat=None if split_stat else self.opt.grad_accum_method)
        self.view_stat = (ViewParallelGradStat(self.flat.params[0].shape[0], self.flat.flat_param.device,
                                               self.opt.grad_accum_method, self.world_size) if split_stat else None)
        self.grad_counter = None  # "mean" accumulation only: per-Gaussian count of views that saw it (train.py:150)
        self._views_checked = set()  # a new Gaussian set: every view's first frame is capacity-checked again
        self._backward_choice_due = True  # ... and the rgb backward kernel is chosen again, behind its first step
        if carry is not None:
            self.optimizer.step_count = int(carry.step_count)
            carry.fill(self.flat, self.optimizer)

    def _view_depth(self, camera, d: Optional[torch.Tensor]):
        """One view's measured depth map as the step uses it -> (range map on the device or None, 1 / its measured pixels):
        the per-view validation and conversion of the constructor and of ``add_view``, stated once."""
        if d is None:
            return None, 0.0
        if d.dtype != torch.float32 or tuple(d.shape) != (int(camera.height), int(camera.width)):
            raise ValueError("a depth map must be float32 [H,W] of its camera")
        d = d.to(self._depth_device)
        if self._depth_kind == "z":
            d = z_to_range(d, camera)
        d = d.contiguous()
        n_valid = int((torch.isfinite(d) & (d > 0)).sum())  # once, here: no count pass in the step
        return d, (1.0 / n_valid if n_valid else 0.0)

    @staticmethod
    def _view_weight(camera, w: Optional[torch.Tensor], device):
        """One view's colour weight map as the step uses it -> (the map on the device or None, (its sum, its sum over the SSIM
        interior) in double): the per-view validation of the constructor and of ``add_view``, stated once.  One host read,
        here: no count pass in the step."""
        if w is None:
            return None, (0.0, 0.0)
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or \
                tuple(w.shape) != (int(camera.height), int(camera.width)):
            raise ValueError("a weight map must be float32 [H,W] of its camera")
        w = w.to(device).contiguous()
        if not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise ValueError("a weight map must be finite and not negative (NaN, inf or a negative weight found)")
        return w, weight_sums(w)

    @staticmethod
    def _view_exposure(camera, exposure, device):
        """One view's exposure (gain, bias) as the step uses it: a fixed ``gs_exposure.Exposure`` of the camera's size."""
        from gs_exposure import Exposure

        gain, bias = exposure
        return Exposure(int(camera.height), int(camera.width), device, gain, bias)

    def add_view(self, camera, target: torch.Tensor, depth: Optional[torch.Tensor] = None,
                 weight: Optional[torch.Tensor] = None, exposure=None) -> int:
        """Appends a view to a running fit -> its camera id.  ``depth`` goes through the constructor's own per-view
        validation and conversion (``depth_kind``, the measured-pixel count); a Trainer built without ``depths`` takes
        ``depth=None`` only.  ``weight``: the view's colour weight map (``weights`` of the constructor; a Trainer built
        without ``weights`` starts its list here, the earlier views without a map).  Nothing else changes -- no rebind, no
        optimizer reset, no frame abandoned: a step on an earlier view afterwards is the step it would have been.  ``exposure`` =
        (gain, bias): the view's affine exposure (``exposures`` of the constructor), held fixed until ``free_exposure``."""
        if depth is not None and self.depths is None:
            raise ValueError("this Trainer was built without depths: add_view takes depth=None only")
        wmap, wsums = self._view_weight(camera, weight, self._depth_device)  # (refused before anything is appended)
        d, inv_n = self._view_depth(camera, depth)
        if exposure is not None:
            self._exposure[len(self.cameras)] = self._view_exposure(camera, exposure, self._depth_device)
        if wmap is not None and self.weights is None:
            self.weights = [None] * len(self.cameras)
            self._weight_sums = [(0.0, 0.0)] * len(self.cameras)
        self.cameras.append(camera)
        self.targets.append(target)
        if self.depths is not None:
            self.depths.append(d)
            self._depth_inv_n.append(inv_n)
        if self.weights is not None:
            self.weights.append(wmap)
            self._weight_sums.append(wsums)
        return len(self.cameras) - 1

    def remove_view(self, camera_id: int):
        """The inverse of ``add_view``: view ``camera_id`` leaves the running fit, and every view above it gets the id one
        lower.  Its entries of ``cameras``, ``targets``, ``depths`` and ``weights`` (where those lists exist) go; the per-view
        keys above it shift down; a frame projected ahead is abandoned.  Parameters, optimizer state, step count and the flat
        bucket are not touched: a step on a remaining view afterwards is the step it would have been.  Refused: the last
        view (``ValueError``) and a view whose pose is free (``RuntimeError``: ``fix_pose`` first)."""
        camera_id = int(camera_id)
        if not 0 <= camera_id < len(self.cameras):
            raise IndexError(f"no view {camera_id}")
        if len(self.cameras) == 1:
            raise ValueError("remove_view would leave the Trainer without a view")
        if camera_id in self._free:
            raise RuntimeError(f"view {camera_id} has a free pose: fix_pose first")
        lists = [self.cameras, self.targets]
        if self.depths is not None:
            lists += [self.depths, self._depth_inv_n]
        if self.weights is not None:
            lists += [self.weights, self._weight_sums]
        for lst in lists:
            del lst[camera_id]
        self._views_checked = {v - (v > camera_id) for v in self._views_checked if v != camera_id}
        self._free = {v - (v > camera_id): fp for v, fp in self._free.items()}
        # (getattr: a Trainer from before `exposures` -- the host tests build one attribute by attribute -- has none)
        self._exposure = {v - (v > camera_id): e for v, e in getattr(self, "_exposure", {}).items() if v != camera_id}
        self.renderer.forward_abandon()  # (a frame projected ahead may have been the removed view's)

    # ------------------------------------------------------------------ free poses (joint refinement of poses and map)
    def free_pose(self, camera_id: int, lr_rot: float, lr_tran: float, betas: Tuple[float, float] = (0.9, 0.999),
                  eps: float = 1e-8):
        """From now on every ``train_step`` on view ``camera_id`` also moves that view's pose: the step's backward delivers
        dL/drot, dL/dtran of the parameters the frame was rendered with (``FrameRenderer.backward_adam(grad_pose=...)``:
        the fused step's pose variant, or ``backward(grad_pose=...)`` + the optimizer where the step cannot be fused), and
        ``gs_track.PoseAdam`` -- the Tracker's optimizer: Adam on the six tangent numbers in float64 on the host, rot <-
        exp([-dw]x) rot -- takes one step on it.  Moments and step count start at zero, the pose at the view's camera.  rgb
        maps only; a step on a free view under view parallelism raises (the slice backward has no pose gradient).

        No host synchronisation in the loop: the 48 bytes travel to pinned memory behind the step, and the pose update is
        applied at the view's NEXT use by any reader (``train_step`` on it, ``seed_from_view``, ``test``, ``pose``,
        ``fix_pose``), which waits for the copy there -- nobody reads the pose in between, so this is exactly eager
        application.  ``cameras[camera_id]`` is then REPLACED by a copy with the new pose in float32: the caller's camera
        object is never written.  A step on a frame that overflowed its pair capacity delivers zero gradients; with Adam's
        moments that still moves the pose, as a zero-gradient step moves a culled Gaussian."""
        from gs_track import _SH_REFUSAL, FreePose, PoseAdam

        rgb = self.flat.params[4]
        if rgb.dim() != 2 or rgb.shape[1] != 3:
            raise RuntimeError(_SH_REFUSAL)
        self._settle_pose(camera_id)
        rot, tran = self.pose(camera_id)
        self._free[camera_id] = FreePose(PoseAdam(rot, tran, lr_rot, lr_tran, betas, eps), self.flat.flat_param.device)

    def fix_pose(self, camera_id: int):
        """Ends ``free_pose``: the pending update is applied, the view keeps the pose it has, its optimizer state is dropped."""
        self._settle_pose(camera_id)
        self._free.pop(camera_id, None)

    def pose(self, camera_id: int):
        """(rot [3,3], tran [3]) of view ``camera_id`` in float64: a free view's own float64 pose (its camera carries the
        float32 rounding of it), else the camera's."""
        self._settle_pose(camera_id)
        fp = self._free.get(camera_id)
        if fp is not None:
            return fp.adam.rot.copy(), fp.adam.tran.copy()
        return pose64(self.cameras[camera_id].rot, self.cameras[camera_id].tran)

    def _settle_pose(self, camera_id):
        """Apply the pose update a free view's last step left pending (waits for that step's 48-byte copy)."""
        fp = self._free.get(camera_id)
        if fp is None or not fp.settle():
            return
        self.cameras[camera_id] = posed(self.cameras[camera_id], fp.adam.rot, fp.adam.tran)

    # ------------------------------------------------------------------ per-view exposure (gs_exposure.Exposure)
    def free_exposure(self, camera_id: int, lr_gain: float, lr_bias: float, betas: Tuple[float, float] = (0.9, 0.999),
                      eps: float = 1e-8):
        """From now on every ``train_step`` on view ``camera_id`` also takes one Adam step on that view's six exposure numbers,
        on the device behind the exposure's backward (no host wait; skipped with the optimizer's step where the frame
        overflowed).  A view without an exposure gets the identity first.  Moments and step count start at zero.  Refused
        under several ranks: each rank would step its own copy."""
        if self.world_size > 1:
            raise RuntimeError("free_exposure is not available under view parallelism (world_size > 1): each rank would step "
                               "its own copy of the exposure")
        camera_id = int(camera_id)
        if not 0 <= camera_id < len(self.cameras):
            raise IndexError(f"no view {camera_id}")
        if camera_id not in self._exposure:
            self._exposure[camera_id] = self._view_exposure(self.cameras[camera_id], (None, None), self.flat.flat_param.device)
        self._exposure[camera_id].free(lr_gain, lr_bias, betas, eps)

    def fix_exposure(self, camera_id: int):
        """Ends ``free_exposure``: the view keeps the exposure it has, its optimizer state is dropped."""
        ex = self._exposure.get(int(camera_id))
        if ex is not None:
            ex.fix()

    def exposure(self, camera_id: int):
        """(gain [3], bias [3]) of view ``camera_id`` in float64 -- one host read --, None for a view without an exposure."""
        ex = self._exposure.get(int(camera_id))
        return ex.values() if ex is not None else None

    @property
    def n_gaussians(self) -> int:
        return int(self.flat.params[0].shape[0])

    def _loss_for(self, h: int, w: int) -> ImageLoss:
        key = (h, w)
        if key not in self._loss:
            self._loss[key] = ImageLoss(h, w, self.opt.ssim_weight, self.flat.flat_param.device)
        return self._loss[key]

    def _weighted_loss_for(self, h: int, w: int) -> WeightedImageLoss:
        key = (h, w)
        if key not in self._weighted_loss:
            self._weighted_loss[key] = WeightedImageLoss(h, w, self.opt.ssim_weight, self.flat.flat_param.device)
        return self._weighted_loss[key]

    def _depth_loss_for(self, h: int, w: int) -> DepthLoss:
        key = (h, w)
        if key not in self._depth_loss:
            self._depth_loss[key] = DepthLoss(h, w, self.opt.depth_mode, self.opt.depth_alpha_min,
                                              self.flat.flat_param.device)
        return self._depth_loss[key]

    def _depth_target(self, camera_id: Optional[int]):
        """The range map this view is supervised with, or None (no maps, no weight, no map for the view)."""
        if self.depths is None or camera_id is None or not self.opt.depth_weight > 0:
            return None
        return self.depths[camera_id]

    def _can_fuse_adam(self) -> bool:
        o, rgb = self.opt, self.flat.params[4]
        return (self.fuse_adam and not self.flat.collective_active() and not self.optimizer.sharded
                and self.view_stat is None and o.scale_reg == 0 and o.opa_reg == 0 and rgb.dim() == 2
                and rgb.shape[1] in (3, 27, 48))

    def _is_control_iteration(self, i_iter: int) -> bool:
        """Does train_step(i_iter) run adaptive_control (prune, or prune + densify)?  train.py:86-91."""
        o = self.opt
        return i_iter > o.adaptive_control_start_iter and i_iter % o.n_adaptive_control == 0

    def train_step(self, i_iter: int, camera_id: int, next_camera_id: Optional[int] = None) -> torch.Tensor:
        """Returns the device tensor (loss, l1, ssim) of this step (no host synchronisation).

        ``next_camera_id``: the view the NEXT step will render, if the caller knows it (a fixed view per rank, a
        pre-drawn camera schedule).  Under view parallelism the project stage of that frame is then issued slice by slice
        behind this step's optimizer, underneath the gradient exchange of the remaining slices (gs_dp.py); the next
        ``train_step`` picks the frame up if it is called with that camera, and renders from scratch otherwise."""
        o = self.opt
        # schedule flags, train.py:86-91
        in_reset = i_iter >= o.n_opa_reset and i_iter % o.n_opa_reset < o.reset_interval
        past = i_iter > o.adaptive_control_start_iter
        only_delete = past and i_iter % o.n_adaptive_control == 0
        control = only_delete and i_iter < o.adaptive_control_end_iter
        accum_start = past and (i_iter + o.grad_accum_iters - 1) % o.n_adaptive_control == 0
        free = self._free.get(camera_id) if self._free else None
        if free is not None:
            if self.flat.collective_active():
                raise RuntimeError(f"view {camera_id} has a free pose: the view-parallel step's slice backward has no pose "
                                   "gradient (fix_pose first, or train on one rank)")
            self._settle_pose(camera_id)  # the pose its previous step left pending
        cam, target = self.cameras[camera_id], self.targets[camera_id]
        flat, r = self.flat, self.renderer
        flat.finish_gather()  # reduce-scatter mode: parameter all-gathers of the previous step that nobody waited for yet
        depth_target = self._depth_target(camera_id)
        depth_map = alpha_map = None
        if depth_target is not None:
            # a depth-supervised view: the frame also renders its depth / alpha maps (never projected ahead: below)
            r.forward_abandon()
            if camera_id not in self._views_checked:
                self._views_checked.add(camera_id)
                r._checked_once = False
            image, _, depth_map, alpha_map = r.forward(*flat.params, cam, aux=True)
        elif r.begun_frame_matches(*flat.params, cam):
            image, _ = r.forward_finish()  # projected behind the previous step's optimizer
        else:
            r.forward_abandon()
            if camera_id not in self._views_checked:  # first frame of this view on this Gaussian set: synchronous check
                self._views_checked.add(camera_id)
                r._checked_once = False
            image, _ = r.forward(*flat.params, cam)
        # a frame that overflowed its workspace all the same was rendered empty: on a single rank the optimizer step
        # is skipped ON THE DEVICE (the fused Adam looks at the frame's overflow counter; no host synchronisation).
        # With several ranks the step is taken -- the other ranks' views still carry gradient, and skipping on one rank
        # would let the replicas drift apart -- and the warning below reports it once the counters arrive.
        self.optimizer.skip_flag = r.overflow_flag() if self.world_size == 1 else None
        if r.overflowed_frames > self._overflow_warned:
            import warnings

            warnings.warn(f"{r.overflowed_frames - self._overflow_warned} training frame(s) exceeded the "
                          f"pair capacity and were rendered empty (single rank: their optimizer steps were skipped on "
                          f"the device; several ranks: this rank contributed zero gradients to them); the "
                          f"workspace has been enlarged to {r.max_pairs} pairs")
            self._overflow_warned = r.overflowed_frames
        wmap = self.weights[camera_id] if self.weights is not None else None
        # a view with an exposure: the colour loss sees the compensated render (the depth loss below never does)
        exposure = self._exposure.get(camera_id) if self._exposure else None
        pred = image if exposure is None else exposure.apply(image)
        if wmap is None:
            loss = self._loss_for(image.shape[0], image.shape[1])
            grad_image = loss(pred, target)
        else:  # a weighted view: the same gradient map travels through whichever backward the step takes
            loss = self._weighted_loss_for(image.shape[0], image.shape[1])
            grad_image = loss(pred, target, wmap, *self._weight_sums[camera_id])
        if exposure is not None:
            # dL/dI' -> dL/dI in place, the six gradients, and a free exposure's Adam step on the device -- skipped, like the
            # optimizer's, where the frame overflowed
            exposure.backward(image, grad_image, skip_flag=self.optimizer.skip_flag)
        # depth supervision: + depth_weight / n_valid * sum |r| on the frame's maps; its two gradient maps travel with
        # grad_image through whichever backward the step takes
        aux_grads = {}
        if depth_target is not None:
            self.depth_loss = self._depth_loss_for(image.shape[0], image.shape[1])
            gd, ga = self.depth_loss(depth_map, alpha_map, depth_target, o.depth_weight * self._depth_inv_n[camera_id])
            aux_grads = {"grad_depth": gd, "grad_alpha": ga}
        if self.densify and accum_start:  # train.py:141-142 (before this step's gradient is accumulated)
            self.optimizer.clear_grad_stat()
            self.grad_counter = None
            if self.view_stat is not None:
                self.view_stat.clear()
        seen = None
        if self.densify and o.grad_accum_method == "mean":
            seen = r.culling_mask().to(torch.float32)

        def local_terms(g0, g1):
            """What needs this rank's OWN gradients of the Gaussians [g0, g1) -- regularisers, the per-view densification
            statistic -- before they are averaged over the ranks."""
            if o.scale_reg > 0:  # train.py:108-109
                sc = flat.params[2]
                flat.grads[2][g0:g1].add_(torch.sign(sc[g0:g1]), alpha=o.scale_reg / sc.numel())
            if self.view_stat is not None:
                self.view_stat.update_range(flat.grads[0], g0, g1)
            if o.opa_reg > 0:  # train.py:110-112
                sg = torch.sigmoid(flat.params[3][g0:g1])
                flat.grads[3][g0:g1].add_(sg * (1 - sg) * (1 - 2 * sg), alpha=o.opa_reg / flat.params[3].numel())

        def settle_backward_choice():
            # One host synchronisation per Gaussian set (the set's first frame was capacity-checked synchronously a moment
            # ago anyway): the backward that has just been issued left the share of its buckets that belong to saturated
            # tiles in the frame's counters; the renderer keeps the rgb backward kernel that share asks for until the next
            # Gaussian set (after a densification the scene is a different one).  Called while THIS frame's descriptor and
            # counters are still the workspace's current ones -- in the view-parallel path that is before the next frame's
            # project stage is issued ahead (behind it the counters may belong to the half-issued frame).
            if self._backward_choice_due:
                self._backward_choice_due = False
                if r.bwd_rows is None and self.flat.params[4].dim() == 2 and self.flat.params[4].shape[1] == 3:
                    r.stats()

        if flat.collective_active():
            # View parallelism.  Every gradient of the frame becomes final in the LAST kernel of the backward, the
            # per-Gaussian sum of the gradient rows; that kernel, the exchange, the optimizer and the NEXT frame's project
            # stage are all independent per Gaussian, so they run as a pipeline over K slices of the Gaussian array:
            #   main stream : rows | S_0 S_1 ... S_K-1 | A_0 P_0 | A_1 P_1 | ...   (S = sums, A = Adam, P = next project)
            #   RCCL stream :        X_0 X_1 ...                                    (X_k starts when S_k is done,
            #                                                                        A_k waits for X_k)
            # Nothing of a slice is applied before its exchange has finished: no stale gradients, the same numbers as
            # the blocking path bit for bit (tests/test_host_logic.py, tests/test_gpu_train.py).
            K = flat.n_slices
            r.backward(grad_image, out=flat.grads, part=_lib.GS_BWD_RASTER, **aux_grads)
            settle_backward_choice()
            if self.view_stat is not None and seen is not None:
                self.view_stat.add_seen(seen)
            for k in range(K):
                g0, g1 = flat.slice_gaussians(k)
                r.backward_slice(flat.grads, g0, g1)
                local_terms(g0, g1)
                flat.begin_slice(k)
            ahead = self._can_project_ahead(i_iter, next_camera_id, control or only_delete)
            lag = 1 if flat.exchange == "reduce_scatter" else 0  # the project needs the GATHERED parameters of its slice
            for k in range(K + lag):
                if k < K:
                    flat.finish_slice(k)
                    self.optimizer.step_slice(k, advance=(k == 0), grad_scale=1.0 / max(self.world_size, 1))
                    flat.begin_slice_gather(k)  # reduce-scatter mode only: the updated shards travel underneath ...
                j = k - lag
                if ahead and j >= 0:
                    flat.finish_slice_gather(j)  # ... the next slice's reduce-scatter + Adam
                    ahead = self._project_ahead(j, next_camera_id)
            # (gathers nobody waited for are waited for where the parameters are read next: finish_gather)
        else:
            # a free pose: the same step with the pose gradient of this frame, written by whichever backward the step takes
            grad_pose = free.grad_pose if free is not None else None
            if self._can_fuse_adam() and (free is None or flat.params[4].shape[1] == 3):
                # one kernel less and no gradient round trip through memory: the per-Gaussian sums, the projection / activation
                # backward and the Adam update of the Gaussian's 14 parameters (+ the |pos.grad| statistic) in one launch
                # (gs_frame_backward_adam; a depth-supervised frame: _adam_aux, the same step with the depth map's position
                # term; a free pose: _adam_pose, rgb maps only -- free_pose refuses others)
                r.backward_adam(grad_image, self.optimizer.fused_descriptor(), grad_pose=grad_pose, **aux_grads)
            else:
                r.backward(grad_image, out=flat.grads, grad_pose=grad_pose, **aux_grads)
                local_terms(0, flat.n)
                if self.view_stat is not None and seen is not None:
                    self.view_stat.add_seen(seen)
                self.optimizer.step()  # also: accum_max_grad = max(|pos.grad|, accum) or += |pos.grad| (train.py:144-153)
            if free is not None:
                with torch.cuda.device(flat.flat_param.device):
                    free.deliver()  # 48 bytes -> pinned host behind the step; read at the view's next use
        if seen is not None and self.view_stat is None:
            self.grad_counter = seen if self.grad_counter is None else self.grad_counter + seen
        settle_backward_choice()
        if self.densify and (control or only_delete):
            self.adaptive_control(i_iter, densify=control and not in_reset)
        # train.py:184-185: the learning rates of the NEXT step
        self.optimizer.set_lrs([f(i_iter) * b for f, b in zip(self._lambdas, self._base)])
        if self.densify and i_iter % o.n_opa_reset == 0 and i_iter > 0:  # train.py:189-190
            from gs_densify import reset_opa

            self.flat.finish_gather()
            self.renderer.forward_abandon()
            reset_opa(self.flat.params[3])
            if self.densify_carry:  # the moments belong to the opacities that were: the original 3DGS optimizer zeroes them too
                for m in self.optimizer.moment_rows("opa"):
                    m.zero_()
        return loss.values

    def tune_slices(self, i_iter: int, camera_id: int, candidates: Sequence[int] = (1, 2, 4), iters: int = 6,
                    next_camera_id: Optional[int] = None) -> int:
        """Pick the number of exchange slices by measurement: ``iters`` real training steps (starting at iteration
        ``i_iter``, all on view ``camera_id``) per candidate, timed with a device synchronisation around each group, the
        slowest rank's time decides (one MAX all-reduce per candidate, so every rank picks the same).  How much wire time
        a further slice hides against what it costs depends on the links, and the builder of this
        code never had more than one GPU: the first steps of a multi-GPU run can settle it themselves.  Replicated
        optimizer ("all_reduce") only.  Returns the chosen count; ``candidates * iters`` steps have been taken."""
        import time

        import torch.distributed as dist

        flat = self.flat
        if not flat.collective_active() or flat.exchange != "all_reduce":
            return flat.n_slices
        o = self.opt
        total = len(candidates) * iters
        if self.densify:
            # a step that runs adaptive_control rebuilds self.flat and the optimizer (_bind), and an opacity
            # reset changes what a step costs -- neither belongs inside a timing comparison.  Refuse a window that holds
            # a control point; the caller tunes between two of them (they are n_adaptive_control iterations apart).
            for it_ in range(i_iter, i_iter + total):
                if self._is_control_iteration(it_) or (it_ % o.n_opa_reset == 0 and it_ > 0):
                    raise RuntimeError(f"tune_slices({i_iter}): iteration {it_} of the {total} tuning steps is a densification "
                                       "/ opacity-reset boundary; start right after one")
        dev = flat.flat_param.device
        best, best_t, it = flat.n_slices, None, i_iter
        for ns in candidates:
            flat = self.flat  # (re-read: nothing below may act on a stale object)
            flat.finish_gather()
            self.renderer.forward_abandon()
            flat.set_slices(ns)
            self.optimizer.reslice()
            self.train_step(it, camera_id, next_camera_id=next_camera_id)  # (first step after a re-slice: views, caches)
            it += 1
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters - 1):
                self.train_step(it, camera_id, next_camera_id=next_camera_id)
                it += 1
            torch.cuda.synchronize(dev)
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
            if self.world_size > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            t = float(t.item())
            if best_t is None or t < best_t:
                best, best_t = flat.n_slices, t
        flat = self.flat
        flat.finish_gather()
        self.renderer.forward_abandon()
        flat.set_slices(best)
        self.optimizer.reslice()
        self.n_slices = best  # a later _bind (densification) keeps the choice
        return best

    def _can_project_ahead(self, i_iter: int, next_camera_id: Optional[int], rebinding: bool) -> bool:
        """May the next frame's project stage be issued behind this step's optimizer?  Only for a view whose capacity
        has been checked on this Gaussian set, and not across a densification / opacity reset (the parameters the
        project stage read would no longer be the ones the frame is rendered with)."""
        o = self.opt
        if next_camera_id is None or next_camera_id not in self._views_checked:
            return False
        if self._depth_target(next_camera_id) is not None:  # rendered with its depth / alpha maps: one call, not in phases
            return False
        if self.densify and (rebinding or (i_iter % o.n_opa_reset == 0 and i_iter > 0)):
            return False
        return True

    def _project_ahead(self, k: int, next_camera_id: int) -> bool:
        """Project stage of the next frame for the Gaussians of exchange slice ``k`` (whole project slices)."""
        flat = self.flat
        per = flat.project_slice
        b0, b1 = flat.slice_bounds[k], min(flat.slice_bounds[k + 1], flat.n)
        if b1 <= b0:
            return True
        ok = self.renderer.forward_begin(*flat.params, self.cameras[next_camera_id], b0 // per, -(-b1 // per),
                                         expect_per_slice=per)
        return ok

    def adaptive_control(self, i_iter: int, densify: bool = True, carry_state: Optional[bool] = None):
        """train.py:156-180: prune (+ clone / split when ``densify``), then a fresh optimizer.
        ``carry_state`` (None: the constructor's ``densify_carry``): the set is edited the way ``prune`` edits it.  Classify,
        the one host read, the draws, then ``gs_densify_apply`` writes the new set straight into the new flat buffer and ONE
        ``gs_densify_apply_state`` moves the ten moment arrays into the new optimizer: a kept or cloned row keeps its moments,
        a split row, the clones and the second samples start from zero, the step count stays.  The statistic is not carried
        (it has just been consumed and restarts at zero, as without carrying); the parameters are the ones the call
        without carrying produces, bit for bit (the draws are taken at the same point, in the same order)."""
        from gs_densify import adaptive_control

        carry = self.densify_carry if carry_state is None else bool(carry_state)
        if carry:
            self._refuse_carry("adaptive_control(carry_state=True)", stat=False)
        o = self.opt
        self.flat.finish_gather()
        if self.view_stat is not None:  # combine the ranks' per-view statistics: one collective per boundary
            accum, cnt = self.view_stat.reduce()
            counter = 1.0 if o.grad_accum_method == "max" else cnt
        else:
            accum = self.optimizer.accum_grad
            counter = 1.0 if o.grad_accum_method == "max" or self.grad_counter is None else self.grad_counter
        stat = accum / (counter + 1e-3 if isinstance(counter, float) else (counter + 1e-3).unsqueeze(-1))  # train.py:160
        if carry:
            with torch.no_grad():
                return self._adaptive_control_carry(i_iter, stat.contiguous(), densify)
        new, counts = adaptive_control(self.flat.params, stat.contiguous(), taus=o.split_thresh,
                                       delete_thresh=o.delete_thresh, scale_activation=self.scale_activation,
                                       grad_thresh=o.grad_thresh, grad_aggregation=o.grad_aggregation,
                                       use_clone=bool(o.use_clone) and densify, use_split=bool(o.use_split) and densify,
                                       clone_dt=o.clone_dt, generator=self.generator)
        self._bind(new, i_iter)
        # the decisions are identical on every rank (same statistic, same parameters), the Gaussian draws of the
        # split are not unless every rank seeds `generator` alike: rank 0's new set is the one that counts
        self.flat.broadcast_params(0)
        return counts

    def _adaptive_control_carry(self, i_iter: int, stat: torch.Tensor, densify: bool):
        """``adaptive_control`` as an edit of the running fit (``carry_state``): no temporary set, the moments travel."""
        from gs_densify import densify_apply, densify_apply_state, densify_classify, densify_draws

        o = self.opt
        old_flat, old_opt = self.flat, self.optimizer
        params, n = [t.detach() for t in old_flat.params], old_flat.n
        counts, ws, opts = densify_classify(params, stat, taus=o.split_thresh, delete_thresh=o.delete_thresh,
                                            scale_activation=self.scale_activation, grad_thresh=o.grad_thresh,
                                            grad_aggregation=o.grad_aggregation, use_clone=bool(o.use_clone) and densify,
                                            use_split=bool(o.use_split) and densify, clone_dt=o.clone_dt)
        kept, cloned, split, total = (int(v) for v in counts.cpu())  # the one host synchronisation
        draws = densify_draws(split, stat.device, self.generator)  # (where gs_densify.adaptive_control draws them)

        def fill(flat, optimizer):
            densify_apply(params, stat, flat.params, counts, ws, opts, draws, split, total)
            torch.autograd.graph.increment_version(flat.flat_param)  # (written through raw pointers, as FusedAdam.step)
            src, dst = [], []
            for name in ("pos", "quat", "scale", "opa", "rgb"):
                src += old_opt.moment_rows(name)
                dst += optimizer.moment_rows(name)
            densify_apply_state(src, dst, n, counts, ws, capacity=total)

        # placeholders give the new flat buffer its shapes; the rows arrive with `fill`, not through a temporary set
        shapes = [torch.empty((total,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device) for t in params]
        self._bind(shapes, i_iter, carry=_Carry(old_opt.step_count, fill))
        self.flat.broadcast_params(0)
        return kept, cloned, split

    def _eval_renderer_for_set(self) -> FrameRenderer:
        """The inference renderer ``test`` and ``seed_from_view`` share (created on first use)."""
        if getattr(self, "_eval_renderer", None) is None:
            self._eval_renderer = FrameRenderer(self.flat.flat_param.device, max_pairs=self.renderer.max_pairs,
                                                training=False, scale_activation=self.scale_activation,
                                                thresh=self.renderer.thresh)
            self._eval_renderer.tile_culling_method = self.renderer.tile_culling_method
            self._eval_renderer.tile_culling_dist_thresh = self.renderer.tile_culling_dist_thresh
        return self._eval_renderer

    def _contrib_renderer_for_set(self) -> FrameRenderer:
        """The second TRAINING renderer ``contributions`` renders its views with (created on first use, sized like the
        evaluation renderer): the fit's own renderer, its workspace, a frame projected ahead in it and its asynchronous
        counters are not touched."""
        if getattr(self, "_contrib_renderer", None) is None:
            self._contrib_renderer = FrameRenderer(self.flat.flat_param.device, max_pairs=self.renderer.max_pairs,
                                                   training=True, scale_activation=self.scale_activation,
                                                   thresh=self.renderer.thresh)
            self._contrib_renderer.tile_culling_method = self.renderer.tile_culling_method
            self._contrib_renderer.tile_culling_dist_thresh = self.renderer.tile_culling_dist_thresh
        return self._contrib_renderer

    @torch.no_grad()
    def contributions(self, camera_ids: Optional[Sequence[int]] = None, w_min: float = CONTRIB_W_MIN) -> Contributions:
        """Each Gaussian's share of the named views (default: all), accumulated into one buffer (``gs_frame.Contributions``:
        weight_sum and pixels summed over the views, weight_max their maximum, ``views`` the number of views in which the
        Gaussian reached ``w_min`` somewhere).  Every view is rendered with a training forward on a renderer of its own; no
        loss, no backward, no optimizer step: a ``train_step`` after this call is the step without it, bit for bit."""
        if self.world_size > 1:
            raise RuntimeError("contributions() is not available under view parallelism (world_size > 1)")
        self.flat.finish_gather()
        ids = list(range(len(self.cameras))) if camera_ids is None else [int(k) for k in camera_ids]
        renderer, params = self._contrib_renderer_for_set(), [t.detach() for t in self.flat.params]
        out = Contributions.empty(self.n_gaussians, self.flat.flat_param.device, w_min)
        for k in ids:
            self._settle_pose(k)
            renderer.forward(*params, self.cameras[k], training=True)
            renderer.contributions(w_min, out=out, accumulate=True)
        return out

    @torch.no_grad()
    def _refuse_carry(self, what: str, stat: bool = True):
        """The optimizer state can travel with the rows only where one rank holds all of it, addressed by row.  ``stat=False``
        (``adaptive_control``, which has just consumed the statistic and carries none): the moments alone decide."""
        optimizer = getattr(self, "optimizer", None)  # (the constructor asks before there is one: FusedAdam.sharded's rule)
        sharded = optimizer.sharded if optimizer is not None else self.exchange == "reduce_scatter"
        if sharded or self.world_size > 1 or (stat and (self.view_stat is not None or self.grad_counter is not None)):
            raise RuntimeError(f"{what} cannot carry the optimizer state of a sharded optimizer (exchange='reduce_scatter'), "
                               "of several ranks (world_size > 1) or of a per-view statistic (per_view_stat, a 'mean' view "
                               "counter): their moments are not row-addressable from one rank; pass carry_state=False")

    @torch.no_grad()
    def prune(self, i_iter: int, *, opa_min: Optional[float] = None, scale_max: Optional[float] = math.inf,
              contributions=None, weight_max_min: float = 0.0, pixels_min: int = 0, views_min: int = 0,
              carry_state: bool = True) -> int:
        """Removes the Gaussians with sigmoid(opa) <= ``opa_min`` or ||act(scale)|| >= ``scale_max`` (``gs_prune``: the delete
        rule of ``adaptive_control`` with both thresholds as arguments; None / inf: no scale test) -> the number removed.
        ``contributions`` (``Trainer.contributions()``) joins the contribution rule to it: a Gaussian also goes when its
        weight_max < ``weight_max_min``, its pixels < ``pixels_min`` or its views < ``views_min`` (``views_min=1``: what reaches
        w_min in no view).  ``opa_min`` may then be None: no opacity test.  Without ``contributions`` the method is what it was
        before the rule existed, and ``opa_min`` is required.
        With ``carry_state`` the kept rows take their Adam moments and their densification statistic with them and the step
        count stays: ONE ``gs_prune_apply`` moves the five parameter arrays, the ten moment arrays and the statistic straight
        into the new flat buffer and the new optimizer's buffers.  ``carry_state=False``: the fresh optimizer of every other
        rebind.  When nothing is removed nothing changes -- no rebind; one host read either way.  A prune that would remove
        every Gaussian is refused.  The Trainer never calls this by itself."""
        from gs_prune import SCALE_ACT, contrib_options, prune_apply, prune_classify, prune_options

        if carry_state:
            self._refuse_carry("prune(carry_state=True)")
        if contributions is None:
            if opa_min is None:
                raise TypeError("prune() needs opa_min (it may be None only with contributions)")
            if weight_max_min or pixels_min or views_min:
                raise ValueError("weight_max_min / pixels_min / views_min need contributions")
            opts = prune_options(opa_min, scale_max, self.scale_activation)
        elif opa_min is None:  # no opacity test: every finite logit lies above the most negative finite float
            opts = _lib.GsPruneOpts(-torch.finfo(torch.float32).max, math.inf if scale_max is None else float(scale_max),
                                    SCALE_ACT[self.scale_activation])
        else:
            opts = prune_options(opa_min, scale_max, self.scale_activation)
        self.flat.finish_gather()
        old_flat, old_opt = self.flat, self.optimizer
        params, n = old_flat.params, old_flat.n
        if contributions is None:
            counts, ws = prune_classify(params[2], params[3], opts)
        else:
            counts, ws = prune_classify(params[2], params[3], opts, contributions,
                                        contrib_options(weight_max_min, pixels_min, views_min))
        kept, removed = (int(v) for v in counts.tolist())  # the one host synchronisation
        if removed == 0:
            return 0
        if kept == 0:
            raise RuntimeError(f"prune(opa_min={opa_min}, scale_max={scale_max}) would remove all {n} Gaussians")
        names = ("pos", "quat", "scale", "opa", "rgb")

        def fill(flat, optimizer):
            src, dst = list(params), list(flat.params)
            if carry_state:
                for name in names:
                    src += old_opt.moment_rows(name)
                    dst += optimizer.moment_rows(name)
                if old_opt.accum_grad is not None:
                    src.append(old_opt.accum_grad)
                    dst.append(optimizer.accum_grad)
            prune_apply(src, dst, n, counts, ws, capacity=kept)

        # placeholders give the new flat buffer its shapes; the rows arrive with `fill`, not through a temporary set
        shapes = [torch.empty((kept,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device) for t in params]
        self._bind(shapes, i_iter, carry=_Carry(old_opt.step_count if carry_state else 0, fill))
        self.flat.broadcast_params(0)
        return removed

    @torch.no_grad()
    def seed_from_view(self, camera_id: int, i_iter: int, carry_state: bool = False, **options) -> int:
        """Extends the Gaussian set by what view ``camera_id`` measured and the current model does not explain
        (``gs_seed.seed_from_depth``: its colour target, its range map, the depth / alpha maps of the current model rendered
        here; ``options``: stride, alpha_thresh, front_rel, scale_factor, opa_init).  Returns the number of Gaussians added.
        A new set gets a fresh optimizer, as after ``adaptive_control``; when nothing is selected nothing changes -- no
        rebind, the optimizer state stays.  ``carry_state=True``: the old rows keep their Adam moments and statistic, the
        appended rows start from zeros, the step count stays (ten block copies, the regions shift in the flat layout).  A new
        row then meets bias corrections near 1 with zero moments: its first update is lr 0.1 g / (0.1 |g| + eps), the
        magnitude of a fresh Adam's first step, so no per-row step count is kept.  The Trainer never calls this by itself: a
        mapping loop calls it per incoming frame, between steps."""
        from gs_seed import seed_from_depth

        if carry_state:
            self._refuse_carry("seed_from_view(carry_state=True)")
        if self.depths is None or self.depths[camera_id] is None:
            raise RuntimeError(f"view {camera_id} has no depth map (Trainer(depths=...)): nothing to seed from")
        self.flat.finish_gather()
        self._settle_pose(camera_id)
        cam, params = self.cameras[camera_id], self.flat.params
        _, _, depth_map, alpha_map = self._eval_renderer_for_set().forward(*params, cam, aux=True)
        n_old = self.n_gaussians
        new = seed_from_depth(self.targets[camera_id], self.depths[camera_id], cam, rendered=(depth_map, alpha_map),
                              color_dim=int(params[4].shape[1]), scale_activation=self.scale_activation,
                              append_to=params, **options)
        added = int(new[0].shape[0]) - n_old
        if added == 0:
            return 0
        carry = None
        if carry_state:
            old_opt = self.optimizer

            def fill(flat, optimizer):
                for name in ("pos", "quat", "scale", "opa", "rgb"):
                    for d, s in zip(optimizer.moment_rows(name), old_opt.moment_rows(name)):
                        d[:n_old].copy_(s)
                if old_opt.accum_grad is not None:
                    optimizer.accum_grad[:n_old].copy_(old_opt.accum_grad)

            carry = _Carry(old_opt.step_count, fill)
        self._bind(new, i_iter, carry=carry)
        self.flat.broadcast_params(0)
        return added

    # ------------------------------------------------------------------ evaluation / viewer hook
    @torch.no_grad()
    def test(self, camera_id, extrinsics=None, intrinsics=None) -> dict:
        """``Trainer.test`` of the reference (train.py:256-281), which is also what its viser GUI calls per
        frame (visergui.py:137-149): ``test(None, extrinsics={"rot", "tran"}, intrinsics={"width", "height",
        "focal_x", "focal_y"[, "cx", "cy"]})`` renders an arbitrary world->camera pose at an arbitrary resolution (the tile
        grid is rebuilt, sizes need not be multiples of 16); ``test(camera_id)`` renders a training / test
        camera and adds ``psnr``, ``ssim`` and ``render_time`` (seconds, device time) against its target."""
        import numpy as np

        from gs_scene import Camera

        self.flat.finish_gather()
        if extrinsics is not None and intrinsics is not None:
            rot, tran = pose64(extrinsics["rot"], extrinsics["tran"])
            cam = Camera(int(intrinsics["width"]), int(intrinsics["height"]), float(intrinsics["focal_x"]),
                         float(intrinsics["focal_y"]), rot.astype(np.float32), tran.astype(np.float32),
                         near=getattr(self.cameras[0], "near", 0.3) if self.cameras else 0.3,
                         cx=intrinsics.get("cx"), cy=intrinsics.get("cy"))  # (optional: the principal point in pixels)
        elif camera_id is not None:
            self._settle_pose(camera_id)
            cam = self.cameras[camera_id]
        else:
            raise RuntimeError("test() needs a camera_id or extrinsics + intrinsics")
        renderer = self._eval_renderer_for_set()
        tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tic.record()
        image, _ = renderer.forward(*self.flat.params, cam)
        toc.record()
        out = {"image": image}
        if camera_id is not None:
            target = self.targets[camera_id]
            toc.synchronize()
            out["render_time"] = tic.elapsed_time(toc) / 1000
            out["psnr"] = self.psnr(image, target)
            h, w = image.shape[:2]
            if h > 10 and w > 10:
                probe = ImageLoss(h, w, 1.0, image.device)  # weight 1: values = (1 - ssim, l1, ssim)
                probe(image, target)
                out["ssim"] = float(probe.values[2])
        return out

    # ------------------------------------------------------------------ checkpoints (train.py:283-291, splatter.py:417-424)
    def save_checkpoint(self, path: str):
        """The reference's ``ckpt.pth``: a dict of the five raw parameter tensors."""
        self.flat.finish_gather()
        pos, quat, scale, opa, rgb = (t.detach().clone() for t in self.flat.params)
        torch.save({"pos": pos, "opa": opa, "rgb": rgb, "quat": quat, "scale": scale}, path)

    def load_checkpoint(self, path: str, i_iter: int = 0):
        ck = torch.load(path, map_location=self.flat.flat_param.device)
        params = [ck[k].detach().to(torch.float32).contiguous() for k in ("pos", "quat", "scale", "opa", "rgb")]
        self._bind(params, i_iter)

    @staticmethod
    def psnr(image: torch.Tensor, target: torch.Tensor) -> float:
        """torchmetrics PeakSignalNoiseRatio() with its default data_range = max(target) - min(target)."""
        mse = torch.mean((image - target) ** 2).item()
        rng = (target.max() - target.min()).item()
        return 10.0 * math.log10(rng * rng / mse) if mse > 0 else float("inf")
