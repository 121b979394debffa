"""gs_exposure_apply / gs_exposure_backward (csrc/exposure.hip, include/gs_abi.h) restated: the maps in numpy float32, one
rounding per operation; the six sums in float64 with their error bound; the Adam step in Python floats, explicit scalar
operations in the kernel's order (a Python float is an IEEE double and the kernel is built without contraction: the two
follow each other operation by operation; sqrt and the power of the bias corrections are each library's own).

    out = apply(image, numbers)                        # numbers = (gain[3], bias[3]) float32
    g, sums, bound = backward(image, grad, numbers)    # the scaled map, the six float64 sums, the bound on each
    state = new_state(); step(state, numbers, grad6, opts, skip=False) -> the new six float32 numbers
"""
import math
import struct

import numpy as np

GAIN_STAR = (0.7, 0.8, 0.9)      # the altered exposure of the fit tests (the issue's)
BIAS_STAR = (0.05, 0.0, -0.03)


def f32(x: float) -> float:
    """``x`` rounded to float32 once (and back)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def numbers(gain=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)) -> np.ndarray:
    return np.asarray(list(gain) + list(bias), np.float32)


def apply(image: np.ndarray, num: np.ndarray) -> np.ndarray:
    """I'_pc = fl(fl(gain_c I_pc) + bias_c): numpy float32 arithmetic rounds every operation once."""
    image, num = np.asarray(image, np.float32), np.asarray(num, np.float32)
    prod = (num[0:3][None, None, :] * image).astype(np.float32)
    return (prod + num[3:6][None, None, :]).astype(np.float32)


def backward(image: np.ndarray, grad: np.ndarray, num: np.ndarray):
    """-> (g = fl(gain g') float32 [H,W,3]; sums float64 [6] = (sum_p g' I per channel, sum_p g' per channel); bound float64 [6]).
    A product of two float32 is exact in double, and ``math.fsum`` adds the terms exactly and rounds once: ``sums`` is the
    float64 sum to half an ulp.  A double sum of n terms in ANY fixed order differs from the exact sum by at most
    (n - 1) 2^-53 sum|term| to first order, which with the reference's own half ulp stays inside n 2^-53 sum|term|: that,
    plus the one rounding to float32 the kernel ends with (2^-24 |sum|; 2^-149 covers a subnormal result)."""
    image, grad, num = np.asarray(image, np.float32), np.asarray(grad, np.float32), np.asarray(num, np.float32)
    g = (num[0:3][None, None, :] * grad).astype(np.float32)
    gi = (grad.astype(np.float64) * image.astype(np.float64)).reshape(-1, 3)
    gb = grad.astype(np.float64).reshape(-1, 3)
    n = image.shape[0] * image.shape[1]
    sums = np.asarray([math.fsum(gi[:, c]) for c in range(3)] + [math.fsum(gb[:, c]) for c in range(3)], np.float64)
    mags = np.asarray([math.fsum(np.abs(gi[:, c])) for c in range(3)] + [math.fsum(np.abs(gb[:, c])) for c in range(3)])
    bound = n * 2.0 ** -53 * mags + 2.0 ** -24 * np.abs(sums) + 2.0 ** -149
    return g, sums, bound


def new_state():
    return {"m": [0.0] * 6, "v": [0.0] * 6, "steps": 0.0}


def default_opts(**kw):
    o = {"lr_gain": 1e-2, "lr_bias": 1e-2, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "lr_scale": 1.0}
    o.update(kw)
    return o


def step(state, num, grad6, opts, skip: bool = False):
    """One Adam step of gs_exposure_backward on the six float32 numbers ``num`` with the six float32 gradients ``grad6`` ->
    the new numbers as a list of Python floats that are float32 values.  ``state`` is updated in place."""
    p = [float(x) for x in num]
    g6 = [float(x) for x in grad6]
    assert len(p) == 6 and len(g6) == 6
    if skip or not all(math.isfinite(x) for x in g6):
        return p
    state["steps"] = state["steps"] + 1.0
    b1, b2 = opts["beta1"], opts["beta2"]
    bc1 = 1.0 - math.pow(b1, state["steps"])
    bc2 = 1.0 - math.pow(b2, state["steps"])
    out = []
    for k in range(6):
        lr = (opts["lr_gain"] if k < 3 else opts["lr_bias"]) * opts["lr_scale"]
        g = g6[k]
        m = b1 * state["m"][k] + (1.0 - b1) * g
        v = b2 * state["v"][k] + ((1.0 - b2) * g) * g
        state["m"][k], state["v"][k] = m, v
        d = (lr * (m / bc1)) / (math.sqrt(v / bc2) + opts["eps"])
        out.append(f32(p[k] - d))
    return out


def tenth_scales():
    """The scale each of the six numbers' errors is held against in the fit tests (a tenth of it): its own starting error from
    the identity, |gain* - 1| and |bias*|; the one number whose starting error is zero (bias* of channel 1) has no scale of
    its own and takes the smallest non-zero one of its group -- the strictest choice the group offers."""
    g = [abs(x - 1.0) for x in GAIN_STAR]
    b = [abs(x) for x in BIAS_STAR]
    b = [x if x > 0 else min(y for y in b if y > 0) for x in b]
    return np.asarray(g + b, np.float64)
