"""Pruning the Gaussian set: remove rows by one per-row decision and move every array that shares the row index.

``prune_rows(scale, opa, arrays, opa_min=..., scale_max=..., scale_activation=...)`` keeps the Gaussians with
sigmoid(opa) > ``opa_min`` and ||act(scale)|| < ``scale_max`` -- the delete rule of ``gs_densify.adaptive_control`` with both
thresholds as arguments -- and returns every array of ``arrays`` (up to sixteen: parameters, optimizer moments, a statistic;
rows of any width) compacted to the kept rows, in order (include/gs_abi.h, gs_prune_classify / gs_prune_apply;
csrc/map_edit.hip).  Three HIP launches and one host read of the counts in between (a control step, like
``gs_seed.seed_from_depth``); bitwise repeatable.  ``gs_train.Trainer.prune`` is the hook that prunes a running fit and takes
its optimizer state along.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace

SCALE_ACT = {"abs": 0, "exp": 1}
# opa_min 0.005: a quarter of the 0.02 the reference prunes below (gs_densify; utils.py:350-351), which it applies inside a
# schedule that also resets opacities; a mapping loop has no such schedule and its seeds start at opa_init = 0.9, so the floor
# only takes what training has driven out of the image.  scale_max inf: no scale test.  No run has been fitted to either.
DEFAULTS = dict(opa_min=0.005, scale_max=math.inf)
MAX_ARRAYS = _lib.GS_PRUNE_MAX_ARRAYS


def opa_logit(p: float) -> float:
    """A probability in (0, 1) as the raw logit the kernel compares, computed in double (inverse_sigmoid, utils.py:350-351)."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"opa_min must lie in (0, 1), got {p!r}")
    return -math.log(1.0 / p - 1.0)


def prune_options(opa_min: float = DEFAULTS["opa_min"], scale_max: Optional[float] = DEFAULTS["scale_max"],
                  scale_activation: str = "abs") -> "_lib.GsPruneOpts":
    return _lib.GsPruneOpts(opa_logit(opa_min), math.inf if scale_max is None else float(scale_max),
                            SCALE_ACT[scale_activation])


def contrib_options(weight_max_min: float = 0.0, pixels_min: int = 0, views_min: int = 0) -> "_lib.GsPruneContribOpts":
    if not float(weight_max_min) >= 0.0:
        raise ValueError(f"weight_max_min must not be NaN or negative, got {weight_max_min!r}")
    if int(pixels_min) < 0 or int(views_min) < 0:
        raise ValueError(f"pixels_min and views_min must not be negative, got {pixels_min!r} and {views_min!r}")
    return _lib.GsPruneContribOpts(float(weight_max_min), int(pixels_min), int(views_min))


def contrib_rows(contributions, n: int) -> torch.Tensor:
    """The raw [N,4] float32 buffer of a ``gs_frame.Contributions`` (or the buffer itself), checked against N."""
    rows = getattr(contributions, "rows", contributions)
    if _rows("contributions", rows, n) != 4 or int(rows.shape[0]) != n:
        raise RuntimeError(f"contributions must hold [{n},4] rows, got {list(rows.shape)}")
    return rows


def _rows(name: str, t: torch.Tensor, n: Optional[int] = None) -> int:
    """A contiguous float32 HIP tensor of rows -> floats per row."""
    check_tensor(name, t, rows_min=0 if n is None else n)
    return int(math.prod(t.shape[1:]))


def prune_classify(scale: torch.Tensor, opa: torch.Tensor, opts, contributions=None,
                   copts=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The decision pass: -> (counts [2] int64 on the device = (kept, removed), workspace).  With ``contributions`` (the rows of
    ``FrameRenderer.contributions``) and ``copts`` (``contrib_options``) the contribution rule is joined to the decision
    (gs_prune_classify_contrib); without them the call is gs_prune_classify."""
    require_hip(scale.device, "pruning")
    n = int(scale.shape[0])
    if _rows("scale", scale) != 3 or _rows("opa", opa) != 1 or int(opa.shape[0]) != n:
        raise RuntimeError(f"scale must be [N,3] and opa [N] of the same N, got {list(scale.shape)} and {list(opa.shape)}")
    ws = workspace(_lib.gs_prune_workspace_bytes(n), scale.device)
    counts = torch.zeros(2, dtype=torch.int64, device=scale.device)
    tail = (counts.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    if contributions is not None:
        rows = contrib_rows(contributions, n)
        _lib.call("gs_prune_classify_contrib", scale.data_ptr(), opa.data_ptr(), rows.data_ptr(), n, C.byref(opts),
                  C.byref(copts if copts is not None else contrib_options()), *tail)
    else:
        _lib.call("gs_prune_classify", scale.data_ptr(), opa.data_ptr(), n, C.byref(opts), *tail)
    return counts, ws


def prune_apply(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], n: int, counts: torch.Tensor, ws: torch.Tensor,
                dst_offset: int = 0, capacity: Optional[int] = None):
    """The move, ONE launch for all arrays: the kept rows of every ``src[k]`` (``n`` rows) become rows [dst_offset, dst_offset +
    kept) of ``dst[k]`` (``capacity`` rows, default: the shortest dst).  Writes nothing if they do not fit."""
    if len(src) != len(dst) or not 1 <= len(src) <= MAX_ARRAYS:
        raise RuntimeError(f"prune_apply moves 1 .. {MAX_ARRAYS} arrays, a dst for every src; got {len(src)} and {len(dst)}")
    cap = min(int(t.shape[0]) for t in dst) if capacity is None else int(capacity)
    a = _lib.GsPruneArrays()
    a.n = len(src)
    for k, (s, d) in enumerate(zip(src, dst)):
        w = _rows(f"src[{k}]", s, int(n))
        if _rows(f"dst[{k}]", d, cap) != w:
            raise RuntimeError(f"array {k}: src rows hold {w} floats, dst rows {_rows('dst', d)}")
        a.width[k], a.src[k], a.dst[k] = max(w, 0), s.data_ptr() or None, d.data_ptr() or None
    _lib.call("gs_prune_apply", C.byref(a), int(n), int(dst_offset), cap, counts.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    # rows written through raw pointers: advance the version counters (a renderer's scene pack is keyed on them)
    torch.autograd.graph.increment_version(tuple(dst))


def prune_rows(scale: torch.Tensor, opa: torch.Tensor, arrays: Sequence[torch.Tensor], *,
               opa_min: float = DEFAULTS["opa_min"], scale_max: Optional[float] = DEFAULTS["scale_max"],
               scale_activation: str = "abs", contributions=None, weight_max_min: float = 0.0, pixels_min: int = 0,
               views_min: int = 0) -> Tuple[List[torch.Tensor], int, int]:
    """-> (the arrays compacted to the kept rows, kept, removed).  ``scale`` [N,3] and ``opa`` [N] decide (raw parameters);
    ``arrays``: up to sixteen float32 tensors of N rows each, ``scale`` and ``opa`` among them if they are to travel.
    ``contributions`` (``FrameRenderer.contributions`` / ``Trainer.contributions``, or their [N,4] buffer) joins the rule
    weight_max >= ``weight_max_min`` and pixels >= ``pixels_min`` and views >= ``views_min`` to the decision; the buffer may
    itself be one of ``arrays``.  Without it the calls are the ones issued before the rule existed."""
    opts = prune_options(opa_min, scale_max, scale_activation)
    n = int(scale.shape[0])
    if contributions is None:
        if weight_max_min or pixels_min or views_min:
            raise ValueError("weight_max_min / pixels_min / views_min need contributions")
        counts, ws = prune_classify(scale, opa, opts)
    else:
        counts, ws = prune_classify(scale, opa, opts, contributions, contrib_options(weight_max_min, pixels_min, views_min))
    kept, removed = (int(v) for v in counts.tolist())  # the one host synchronisation
    out = [torch.empty((kept,) + tuple(t.shape[1:]), dtype=torch.float32, device=scale.device) for t in arrays]
    if kept:
        prune_apply([t.detach() for t in arrays], out, n, counts, ws)
    return out, kept, removed
