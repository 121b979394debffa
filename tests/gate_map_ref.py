"""Reference statements of gs_track_gate_mask and gs_loss_l1_ssim_weighted (include/gs_abi.h) for tests/test_gate_map_host.py
and tests/test_gpu_gate_map.py -- a helper, not a test: the mask contract from the float32 residual maps and the gate of
tests/track_gate_ref.py, and a float64 weighted L1 + SSIM with its gradient built from the filters of oracle/train_ref.py."""
import numpy as np

from oracle.train_ref import _filt_full_adjoint, _filt_valid, gaussian_window
from track_gate_ref import gate_from_residuals, residuals_f32


def interior(H, W):
    """The SSIM interior as a bool map: rows 5 .. H-6, columns 5 .. W-6; empty when H <= 10 or W <= 10."""
    m = np.zeros((H, W), bool)
    if H > 10 and W > 10:
        m[5:H - 5, 5:W - 5] = True
    return m


def gate_mask_ref(I, D, A, T, z, alpha_min, k_d, k_c, floor_d=0.0, floor_c=0.0, couple=True):
    """gs_track_gate_mask decided in float32 -> (range_out or None, weight_out, the eight values as float32, the gate dict).
    ``z`` None: an RGB-only gate."""
    ra, rc, covered, meas = residuals_f32(I, D, A, T, z, alpha_min)
    g = gate_from_residuals(ra, rc, covered, meas, k_d, k_c, floor_d, floor_c, couple)
    removed = covered & meas & ~g["dmask"]
    kept = meas & ~removed
    rng = None if z is None else np.where(kept, np.asarray(z, np.float32), np.float32(0)).astype(np.float32)
    weight = np.where(covered & ~g["cmask"], np.float32(0), np.float32(1)).astype(np.float32)
    H, W = weight.shape
    values = np.array([meas.sum(), kept.sum(), removed.sum(), weight.sum(dtype=np.float64),
                       weight[interior(H, W)].sum(dtype=np.float64), g["m_d"], g["m_c"], g["n_d"]], np.float32)
    return rng, weight, values, g


def weight_sums(weight):
    """(sum of the map, its sum over the SSIM interior) in float64: the two host arguments of the weighted loss."""
    m = np.asarray(weight, np.float64)
    return float(m.sum()), float(m[interior(*m.shape)].sum())


def weighted_l1_ssim_loss(pred, target, weight, ssim_weight=0.1, dtype=np.float64):
    """(loss, l1, ssim, dloss/dpred) of gs_loss_l1_ssim_weighted for [H,W,3] images and a [H,W] weight map:
    l1 = sum m |x - y| / (3 sum m), ssim = sum_interior m S / (3 sum_interior m), loss = (1 - w) l1 + w (1 - ssim); a term
    whose weights sum to zero is zero, value and gradient."""
    x, y, m = np.asarray(pred, dtype), np.asarray(target, dtype), np.asarray(weight, dtype)
    H, W, _ = x.shape
    ws, wsi = m.sum(), (m[5:H - 5, 5:W - 5].sum() if H > 10 and W > 10 else 0.0)
    l1, grad = 0.0, np.zeros_like(x)
    if ws > 0:
        l1 = (m[:, :, None] * np.abs(x - y)).sum() / (3.0 * ws)
        grad = (1.0 - ssim_weight) * m[:, :, None] * np.sign(x - y) / (3.0 * ws)
    ssim, term = 0.0, 0.0
    if ssim_weight > 0 and wsi > 0:
        g = gaussian_window(dtype=dtype)
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        mu, nu = _filt_valid(x, g), _filt_valid(y, g)
        exx, eyy, exy = _filt_valid(x * x, g), _filt_valid(y * y, g), _filt_valid(x * y, g)
        vx_raw, vy_raw = exx - mu * mu, eyy - nu * nu
        vx, vy = np.maximum(vx_raw, 0), np.maximum(vy_raw, 0)
        A1, A2 = 2 * mu * nu + c1, 2 * (exy - mu * nu) + c2
        B1, B2 = mu * mu + nu * nu + c1, vx + vy + c2
        S = A1 * A2 / (B1 * B2)
        mi = m[5:H - 5, 5:W - 5, None]
        ssim = (mi * S).sum() / (3.0 * wsi)
        dExx = np.where(vx_raw > 0, -S / B2, 0.0)
        dmu = 2 * nu * (A2 - A1) / (B1 * B2) - 2 * mu * S / B1 - 2 * mu * dExx
        dExy = 2 * A1 / (B1 * B2)
        dS_dx = _filt_full_adjoint(mi * dmu, g, H, W) + 2 * x * _filt_full_adjoint(mi * dExx, g, H, W) \
            + y * _filt_full_adjoint(mi * dExy, g, H, W)
        grad = grad - ssim_weight * dS_dx / (3.0 * wsi)
        term = ssim_weight * (1.0 - ssim)
    return float((1.0 - ssim_weight) * l1 + term), float(l1), float(ssim), grad
