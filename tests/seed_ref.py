"""NumPy restatement of seeding from an RGB-D frame (include/gs_abi.h, gs_seed_classify / gs_seed_apply), for the tests.

The DECISION is restated in float32, one rounding per operation, as the kernel is specified: it must select exactly the
kernel's pixels.  What a selected pixel BECOMES is restated in float64 from the same float32 inputs: closed forms the
kernel's fp32 arithmetic is held against within a bound counted from its operations."""
import math

import numpy as np

COLOR_MIN = 1.0 / 512.0
SH_C0 = 0.28209479177387814


def lattice(H, W, stride):
    """(ys, xs) of the lattice pixels, x % stride == stride // 2 and y % stride == stride // 2, in row-major order."""
    off = stride // 2
    ys, xs = np.meshgrid(np.arange(off, H, stride), np.arange(off, W, stride), indexing="ij")
    return ys.reshape(-1), xs.reshape(-1)


def select(z, D, A, stride, alpha_thresh, front_rel):
    """-> (selected, measured), boolean [H,W] maps that are False off the lattice.  D = A = None: no maps."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    on = np.zeros((H, W), bool)
    ys, xs = lattice(H, W, stride)
    on[ys, xs] = True
    with np.errstate(invalid="ignore", over="ignore"):
        meas = on & (z > np.float32(0)) & (z <= np.finfo(np.float32).max)
        if D is None:
            return meas.copy(), meas
        A, D = np.asarray(A, np.float32), np.asarray(D, np.float32)
        keep = np.float32(1.0) - np.float32(front_rel)  # one rounding
        lhs = (z * A).astype(np.float32)
        rhs = (keep * D).astype(np.float32)
        sel = meas & ((A < np.float32(alpha_thresh)) | (lhs < rhs))
    return sel, meas


def pixel_rays(cam, ys, xs):
    """(u, v) of the renderer's ray through the centres of the pixels (ys, xs) of the cropped image, in float64 from the
    float32 focal lengths: ((x + left - padW / 2 + 0.5) / fx, (y + top - padH / 2 + 0.5) / fy)."""
    W, H = int(cam.width), int(cam.height)
    padW, padH = -(-W // 16) * 16, -(-H // 16) * 16
    left, top = (padW - W) // 2, (padH - H) // 2
    fx, fy = float(np.float32(cam.focal_x)), float(np.float32(cam.focal_y))
    return (xs + left - padW / 2 + 0.5) / fx, (ys + top - padH / 2 + 0.5) / fy


def gaussians(image, z, cam, sel, stride, scale_factor, opa_init, color_dim=3):
    """float64 closed forms for the selected pixels in row-major order: dict of pos [n,3], sigma [n] (the ACTIVATED scale),
    z_cam [n], opa (the logit), logit [n,3] (the colour logits), rgb [n,color_dim], reach [n] = range + |tran|."""
    ys, xs = np.nonzero(sel)  # row-major
    u, v = pixel_rays(cam, ys, xs)
    rng = np.asarray(z, np.float32)[ys, xs].astype(np.float64)
    z_cam = rng / np.sqrt(u * u + v * v + 1.0)
    p_c = np.stack([u * z_cam, v * z_cam, z_cam], 1)
    rot = np.asarray(cam.rot, np.float32).astype(np.float64).reshape(3, 3)
    tran = np.asarray(cam.tran, np.float32).astype(np.float64).reshape(3)
    pos = (p_c - tran) @ rot  # rot^T (p_c - tran) per row
    fx, fy = float(np.float32(cam.focal_x)), float(np.float32(cam.focal_y))
    sigma = float(np.float32(scale_factor)) * stride * z_cam / ((fx + fy) / 2)
    c = np.clip(np.asarray(image, np.float32)[ys, xs].astype(np.float64), COLOR_MIN, 1.0 - COLOR_MIN)
    logit = np.log(c / (1.0 - c))
    if color_dim == 3:
        rgb = logit
    else:
        nb = color_dim // 3
        rgb = np.zeros((len(ys), 3, nb))
        rgb[:, :, 0] = logit / float(np.float32(SH_C0))
        rgb = rgb.reshape(len(ys), color_dim)
    p = float(np.float32(opa_init))
    return dict(pos=pos, sigma=sigma, z_cam=z_cam, opa=-math.log(1.0 / p - 1.0), logit=logit, rgb=rgb,
                reach=rng + np.linalg.norm(tran), ys=ys, xs=xs)
