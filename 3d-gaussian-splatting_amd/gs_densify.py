"""Densification: the reference's ``Gaussian3ds.adaptive_control`` / ``reset_opa`` (splatter.py:119-228).

``adaptive_control(params, grad, ...)`` takes the five parameter tensors (pos, quat, scale, opa, rgb) and the
accumulated position-gradient statistic, and returns the five tensors of the new Gaussian set in the
reference's order: kept Gaussians (pruned by opacity / size; the ones that are split get ``scale / 1.6``
and a fresh sample), then the clones, then the second split samples.  Two HIP launches classify and count,
one applies; the only host synchronisation is the read of the four counts between them (the reference
synchronises four times and launches ~40 torch kernels).  The optimizer state is dropped afterwards, as in
the reference, which re-creates ``torch.optim.Adam`` (train.py:169-179).

The two halves are stated once, ``densify_classify`` and ``densify_apply``; ``adaptive_control`` is the two around the host
read and the draws.  A caller that edits a running fit in place (``gs_train.Trainer.adaptive_control(carry_state=True)``)
takes the halves apart, applies straight into its own buffers and lets ``densify_apply_state`` move whatever shares the row
index -- Adam's moments -- the same way (gs_densify_apply_state, include/gs_abi.h).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace
from gs_prune import MAX_ARRAYS, _rows

SCALE_ACT = {"abs": 0, "exp": 1}
AGG = {"max": 0, "mean": 1}


def inverse_sigmoid(y: float) -> float:  # utils.py:350-351
    return -math.log(1 / y - 1)


def densify_classify(params: Sequence[torch.Tensor], grad: torch.Tensor, taus: float, delete_thresh: float,
                     scale_activation: str = "abs", grad_thresh: float = 0.0002, grad_aggregation: str = "max",
                     use_clone: bool = True, use_split: bool = True, clone_dt: float = 0.01):
    """The decision pass (two launches, no host read): -> (counts [4] int64 on the device = (kept, cloned, split, total),
    workspace, opts).  All three go to ``densify_apply`` / ``densify_apply_state`` as they are."""
    pos, quat, scale, opa, rgb = params
    n = int(pos.shape[0])
    dev = require_hip(pos.device, "adaptive_control")
    color_dim = int(rgb.shape[1])
    for name, t, shape in (("pos", pos, (n, 3)), ("quat", quat, (n, 4)), ("scale", scale, (n, 3)), ("opa", opa, (n,)),
                           ("rgb", rgb, (n, color_dim)), ("grad", grad, (n, 3))):
        check_tensor(name, t, shape)
    opts = _lib.GsDensifyOpts(float(taus), float(delete_thresh), float(grad_thresh), float(clone_dt),
                              SCALE_ACT[scale_activation], AGG[grad_aggregation], int(bool(use_clone)),
                              int(bool(use_split)), color_dim)
    ws = workspace(_lib.gs_densify_workspace_bytes(n), dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.call("gs_densify_classify", scale.data_ptr(), opa.data_ptr(), grad.data_ptr(), n, C.byref(opts), counts.data_ptr(),
              ws.data_ptr(), ws.numel(), stream())
    return counts, ws, opts


def densify_draws(split: int, device, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MultivariateNormal.sample() twice (utils.py:396-401): two [n_split, 3] normal blocks, drawn in this order."""
    return tuple(torch.randn(split, 3, device=device, generator=generator) for _ in range(2))


def densify_apply(params: Sequence[torch.Tensor], grad: torch.Tensor, out: Sequence[torch.Tensor], counts: torch.Tensor,
                  ws: torch.Tensor, opts, draws: Tuple[torch.Tensor, torch.Tensor], split: int, capacity: int):
    """The edit, one launch: the new set of ``densify_classify``'s decision into the five tensors ``out`` (``capacity`` rows
    each).  ``draws`` = (eps1, eps2), two [>= split, 3] standard-normal tensors.  Writes nothing if the set does not fit."""
    eps1, eps2 = (d.contiguous() for d in draws)
    if eps1.shape[0] < split or eps2.shape[0] < split:
        raise RuntimeError(f"need {split} normal draws per block, got {eps1.shape[0]}, {eps2.shape[0]}")
    pos, quat, scale, opa, rgb = params
    _lib.call("gs_densify_apply", pos.data_ptr(), quat.data_ptr(), scale.data_ptr(), opa.data_ptr(), rgb.data_ptr(),
              grad.data_ptr(), int(pos.shape[0]), C.byref(opts), eps1.data_ptr(), eps2.data_ptr(),
              min(int(eps1.shape[0]), int(eps2.shape[0])), *(t.data_ptr() for t in out), int(capacity), counts.data_ptr(),
              ws.data_ptr(), ws.numel(), stream())


def densify_apply_state(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], n: int, counts: torch.Tensor,
                        ws: torch.Tensor, capacity: Optional[int] = None):
    """What shares the row index follows the edit, ONE launch for all arrays (gs_densify_apply_state): of every ``src[k]``
    (``n`` rows) the kept and the cloned rows go to their kept rank in ``dst[k]``; the kept slot of a split row, the clones'
    rows and the second samples' rows become zero.  ``counts`` and ``ws`` are ``densify_classify``'s for these rows;
    ``capacity``: rows of every dst (default: the shortest).  Writes nothing if the new set does not fit."""
    if len(src) != len(dst) or not 1 <= len(src) <= MAX_ARRAYS:
        raise RuntimeError(f"densify_apply_state moves 1 .. {MAX_ARRAYS} arrays, a dst for every src; got {len(src)} and "
                           f"{len(dst)}")
    require_hip(counts.device, "densify_apply_state")
    cap = min(int(t.shape[0]) for t in dst) if capacity is None else int(capacity)
    a = _lib.GsPruneArrays()
    a.n = len(src)
    for k, (s, d) in enumerate(zip(src, dst)):
        w = _rows(f"src[{k}]", s, int(n))
        if _rows(f"dst[{k}]", d, cap) != w:
            raise RuntimeError(f"array {k}: src rows hold {w} floats, dst rows {_rows('dst', d)}")
        a.width[k], a.src[k], a.dst[k] = max(w, 0), s.data_ptr() or None, d.data_ptr() or None
    _lib.call("gs_densify_apply_state", C.byref(a), int(n), cap, counts.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.autograd.graph.increment_version(tuple(dst))  # (rows written through raw pointers, as gs_prune.prune_apply)


def adaptive_control(params: Sequence[torch.Tensor], grad: torch.Tensor, taus: float, delete_thresh: float,
                     scale_activation: str = "abs", grad_thresh: float = 0.0002, grad_aggregation: str = "max",
                     use_clone: bool = True, use_split: bool = True, clone_dt: float = 0.01,
                     generator: Optional[torch.Generator] = None,
                     draws: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                     ) -> Tuple[List[torch.Tensor], Tuple[int, int, int]]:
    """Returns ([pos, quat, scale, opa, rgb] of the new set, (kept, cloned, split)).

    ``draws`` = (eps1, eps2), two [>= n_split, 3] standard-normal tensors, replaces the internal
    ``torch.randn`` (tests replay the reference's draws with it)."""
    counts, ws, opts = densify_classify(params, grad, taus, delete_thresh, scale_activation, grad_thresh, grad_aggregation,
                                        use_clone, use_split, clone_dt)
    dev = params[0].device
    kept, cloned, split, total = (int(v) for v in counts.cpu())  # the one host synchronisation
    if draws is None:
        draws = densify_draws(split, dev, generator)
    out = [torch.empty((total,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in params]
    densify_apply(params, grad, out, counts, ws, opts, draws, split, total)
    return out, (kept, cloned, split)


def reset_opa(opa: torch.Tensor) -> torch.Tensor:
    """splatter.py:119-120: every opacity logit back to logit(0.01)."""
    return opa.fill_(inverse_sigmoid(0.01))
