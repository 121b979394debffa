"""The plumbing around a call into libgs_amd.so, stated once: the refusal of a non-HIP device, the check of a tensor argument,
the workspace buffer and the current stream.  (The call itself is ``gaussian._lib.call``.)  Imports neither ``gs_frame`` nor
anything that needs a device.
"""
from __future__ import annotations

import torch


def require_hip(device, who: str):
    """``device`` (a name or a device) as a device; every kernel is HIP, so any other kind is refused in ``who``'s name."""
    device = torch.device(device) if isinstance(device, (str, int)) else device
    if device.type != "cuda":
        raise RuntimeError(f"{who} needs a HIP device; there is no CPU fallback")
    return device


def _shape(dims) -> str:
    return "[" + ", ".join(str(d) for d in dims) + "]"


def check_tensor(name: str, t: torch.Tensor, shape=None, *, rows_min=None, tail=None, device=None) -> torch.Tensor:
    """``t`` if it is a contiguous float32 HIP tensor that meets the shape rule: exactly ``shape``; or at least ``rows_min`` rows
    of row shape ``tail`` (None: rows of any shape); or no rule.  ``device``: it must also live there."""
    ok = t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and (device is None or t.device == device)
    rule = ""
    if shape is not None:
        rule = f" of shape {_shape(shape)}"
        ok = ok and tuple(t.shape) == tuple(shape)
    elif rows_min is not None:
        rule = f" of shape {_shape((f'>= {rows_min}',) + (('...',) if tail is None else tuple(tail)))}"
        ok = ok and t.dim() >= 1 and t.shape[0] >= rows_min and (tail is None or tuple(t.shape[1:]) == tuple(tail))
    if not ok:
        where = f" on the same device as {device}" if device is not None else ""
        raise RuntimeError(f"{name} must be a contiguous float32 HIP tensor{rule}{where}")
    return t


def workspace(nbytes, device, floor: int = 0) -> torch.Tensor:
    """The uint8 buffer a ``gs_*_workspace_bytes`` answer asks for (at least ``floor`` bytes)."""
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)


def stream():
    """The current HIP stream as the library takes it."""
    return torch.cuda.current_stream().cuda_stream
