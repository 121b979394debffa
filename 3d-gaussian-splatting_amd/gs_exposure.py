"""A view's affine exposure: six numbers, ``gain[3]`` and ``bias[3]`` per colour channel, between the rendered image and any
of the colour losses (gs_exposure_apply / gs_exposure_backward, csrc/exposure.hip, include/gs_abi.h).

    compensated = exposure.apply(image)          # I' = fl(fl(gain I) + bias); the loss is taken on I' in place of I
    grad = loss(compensated, ...)                # any loss kernel: g' = dL/dI'
    exposure.backward(image, grad)               # grad <- fl(gain g') in place, .grad <- (dL/dgain, dL/dbias); steps when free

The six numbers live in device memory and the kernels read them as they stand when they run; ``free`` gives them an Adam
state on the device (double) and every ``backward`` then takes one step behind the sums, with no host wait.  Depth and
alpha terms never see the exposure.  The identity leaves image and gradient bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace

IDENTITY = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)


def numbers32(gain=None, bias=None) -> np.ndarray:
    """(gain, bias) -- None: the identity's -- as the six float32 the device holds, gain first; finite numbers only."""
    g = np.ones(3) if gain is None else np.asarray(gain, np.float64).reshape(-1)
    b = np.zeros(3) if bias is None else np.asarray(bias, np.float64).reshape(-1)
    if g.shape != (3,) or b.shape != (3,):
        raise ValueError("an exposure is gain[3] and bias[3], one pair per colour channel")
    x = np.concatenate([g, b])
    if not np.isfinite(x).all():
        raise ValueError("gain and bias must be finite")
    return x.astype(np.float32)


class _Fit:
    """What the ``Exposure`` objects of one view share (``Exposure.sibling``: the levels of a pyramid): the six numbers, their
    gradient, and -- while free -- the Adam state and its rates."""

    def __init__(self, numbers: torch.Tensor):
        self.numbers = numbers
        self.grad = torch.zeros(6, dtype=torch.float32, device=numbers.device)
        self.state: Optional[torch.Tensor] = None  # gs_exposure_state: m[6], v[6], steps in double
        self.rates = None                          # (lr_gain, lr_bias, beta1, beta2, eps)


class Exposure:
    """``Exposure(height, width, device, gain=None, bias=None)``: owns the six numbers (``numbers``, float32 on the device,
    gain first), the compensated image, the workspace and, after ``free``, the Adam state.  ``numbers=``: six contiguous
    float32 on the device to adopt in place of an allocation (a caller that reads them with other values in one copy)."""

    def __init__(self, height: int, width: int, device="cuda", gain=None, bias=None, numbers: Optional[torch.Tensor] = None,
                 _fit: Optional[_Fit] = None):
        self.H, self.W = int(height), int(width)
        if self.H <= 0 or self.W <= 0:
            raise ValueError("an exposure needs an image of positive size")
        self.device = require_hip(device, "Exposure")
        init = numbers32(gain, bias)  # (refused before anything is allocated)
        if _fit is None:
            if numbers is None:
                numbers = torch.zeros(6, dtype=torch.float32, device=self.device)
            elif check_tensor("numbers", numbers).numel() != 6:
                raise RuntimeError("numbers must hold 6 floats")
            _fit = _Fit(numbers)
            _fit.numbers.copy_(torch.from_numpy(init))
        self._fit = _fit
        self.device = self._fit.numbers.device
        self.out = torch.empty(self.H, self.W, 3, dtype=torch.float32, device=self.device)
        self._ws = workspace(_lib.gs_exposure_workspace_bytes(self.H, self.W), self.device)

    def sibling(self, height: int, width: int) -> "Exposure":
        """The same exposure for images of another size: buffers of its own, the same six numbers, gradient and Adam state."""
        return Exposure(height, width, self.device, _fit=self._fit)

    @property
    def numbers(self) -> torch.Tensor:
        return self._fit.numbers

    @property
    def grad(self) -> torch.Tensor:
        """(dL/dgain[3], dL/dbias[3]) of the last ``backward``, on the device."""
        return self._fit.grad

    @property
    def is_free(self) -> bool:
        return self._fit.state is not None

    def set(self, gain=None, bias=None):
        """Replace the six numbers (one 24-byte copy); a free exposure's Adam state starts over."""
        self._fit.numbers.copy_(torch.from_numpy(numbers32(gain, bias)))
        if self._fit.state is not None:
            self._fit.state.zero_()

    def free(self, lr_gain: float, lr_bias: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        """From now on every ``backward`` also takes one Adam step on the six numbers, on the device.  Moments and step count
        start at zero."""
        rates = (float(lr_gain), float(lr_bias), float(betas[0]), float(betas[1]), float(eps))
        if not all(np.isfinite(r) and r >= 0 for r in rates) or not (rates[2] < 1 and rates[3] < 1):
            raise ValueError("lr_gain, lr_bias and eps must be finite and not negative, the betas must lie in [0, 1)")
        self._fit.rates = rates
        self._fit.state = torch.zeros(C.sizeof(_lib.GsExposureState) // 8, dtype=torch.float64, device=self.device)

    def fix(self):
        """Ends ``free``: the numbers stay what they are, the Adam state is dropped."""
        self._fit.state = self._fit.rates = None

    def apply(self, image: torch.Tensor) -> torch.Tensor:
        """``image`` [H,W,3] -> the compensated image (``self.out``, rewritten by the next call)."""
        check_tensor("image", image, (self.H, self.W, 3))
        _lib.call("gs_exposure_apply", image.data_ptr(), self._fit.numbers.data_ptr(), self.H, self.W, self.out.data_ptr(),
                  stream())
        return self.out

    def backward(self, image: torch.Tensor, grad: torch.Tensor, lr_scale: float = 1.0, skip_flag=None) -> torch.Tensor:
        """``image``: what ``apply`` took; ``grad`` [H,W,3] = dL/d(compensated), scaled in place to dL/d(image) and returned.
        Fills ``self.grad`` and, when free, steps the six numbers at ``lr_scale`` x the rates unless the 64-bit device counter
        at address ``skip_flag`` (``FusedAdam.skip_flag``) is non-zero."""
        check_tensor("image", image, (self.H, self.W, 3))
        check_tensor("grad", grad, (self.H, self.W, 3))
        f = self._fit
        adam = None
        if f.state is not None:
            lg, lb, b1, b2, eps = f.rates
            adam = C.byref(_lib.GsExposureAdam(f.state.data_ptr(), lg, lb, b1, b2, eps, float(lr_scale), skip_flag))
        _lib.call("gs_exposure_backward", image.data_ptr(), grad.data_ptr(), f.numbers.data_ptr(), self.H, self.W,
                  f.grad.data_ptr(), adam, self._ws.data_ptr(), self._ws.numel(), stream())
        return grad

    def values(self) -> Tuple[np.ndarray, np.ndarray]:
        """(gain [3], bias [3]) as float64 arrays: the one host read."""
        x = self._fit.numbers.cpu().numpy().astype(np.float64)
        return x[0:3].copy(), x[3:6].copy()
