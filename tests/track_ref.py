"""Reference statements of gs_loss_track (include/gs_abi.h) for tests/test_track_host.py and tests/test_gpu_track.py -- a
helper, not a test: a float64 evaluation of the contract, a float32 restatement of the colour gradient (which the contract
makes exactly reproducible), the inputs of the loss tests, and the SE(3) helpers of the tracker tests."""
import math

import numpy as np


def measured(z):
    """The "no measurement" rule of gs_loss_depth: <= 0, infinite and NaN carry no measurement."""
    z = np.asarray(z)
    return np.isfinite(z) & (np.where(np.isfinite(z), z, 0.0) > 0)


def track_loss_f64(I, D, A, T, z, alpha_min, color_weight, depth_weight, depth_gate, scale):
    """gs_loss_track in float64 on the float32 inputs.  ``z`` None: RGB only.  -> dict with the three gradients, the three
    values, the depth count, r, the masks (colour, depth) and ``undecidable``: the measured pixels inside the silhouette
    whose sign of r, or whose gate decision, an fp32 evaluation cannot be asked to reproduce -- |r| (or its distance from the
    gate) below 1e-6 max(|D / A|, |z|), where fp32 computes D / A and the difference with a relative error of 2^-24 each."""
    I, D, A, T = (np.asarray(a, np.float64) for a in (I, D, A, T))
    H, W = A.shape
    cmask = A >= float(np.float32(alpha_min))
    cs, ds = float(scale) * float(color_weight), float(scale) * float(depth_weight)
    diff = I - T
    g_img = np.where(cmask[:, :, None], cs * np.sign(diff), 0.0)
    colour = cs * float(np.abs(diff)[cmask].sum())
    g_d, g_a = np.zeros((H, W)), np.zeros((H, W))
    r = np.zeros((H, W))
    dmask = np.zeros((H, W), bool)
    undecidable = np.zeros((H, W), bool)
    if z is not None:
        z = np.asarray(z, np.float64)
        inside = cmask & measured(z)
        zz = np.where(inside, z, 1.0)
        Aa = np.where(inside, A, 1.0)
        e = D / Aa
        r = np.where(inside, e - zz, 0.0)
        mag = 1e-6 * np.maximum(np.abs(e), np.abs(zz))
        undecidable = inside & (np.abs(r) < mag)
        dmask = inside.copy()
        if depth_gate > 0:
            g = float(np.float32(depth_gate))
            dmask &= np.abs(r) <= g
            undecidable |= inside & (np.abs(np.abs(r) - g) < mag)
        g_d = np.where(dmask, ds * np.sign(r) / Aa, 0.0)
        g_a = np.where(dmask, -ds * np.sign(r) * e / Aa, 0.0)
    depth = ds * float(np.abs(r)[dmask].sum())
    return dict(grad_image=g_img, grad_depth=g_d, grad_alpha=g_a, loss=colour + depth, colour=colour, depth=depth,
                count=int(dmask.sum()), r=r, cmask=cmask, dmask=dmask, undecidable=undecidable)


def colour_grad_f32(I, T, A, alpha_min, color_weight, scale):
    """grad_image as the kernel computes it, in float32: +-fl(scale color_weight) by the sign of the fp32 difference (which
    is the exact sign), 0 where equal or outside the silhouette."""
    I, T, A = (np.asarray(a, np.float32) for a in (I, T, A))
    cs = np.float32(np.float32(scale) * np.float32(color_weight))
    d = I - T
    g = np.where(d > 0, cs, np.where(d < 0, -cs, np.float32(0))).astype(np.float32)
    return np.where((A >= np.float32(alpha_min))[:, :, None], g, np.float32(0)).astype(np.float32)


# the sizes of the loss test with the seeds of their inputs and the gate (which cuts roughly a tenth of the measured pixels)
LOSS_CASES = [(7, 9, 16), (48, 64, 112), (187, 250, 437), (1080, 1920, 3000)]
ALPHA_MIN, GATE = 0.5, 2.0


def loss_inputs(H, W, seed, all_measured=False):
    """After tests/test_gpu_rgbd.py::_loss_inputs: A straddles alpha_min = 0.5, 30 % of z carries no measurement in each of
    the four ways, D / A - z = z U(-0.3, 0.3); image and target in [0, 1] with a tenth of the entries exactly equal."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.02, 1.0, (H, W)).astype(np.float32)
    z = rng.uniform(0.3, 12.0, (H, W)).astype(np.float32)
    D = (A * z * rng.uniform(0.7, 1.3, (H, W))).astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.30
    kind = rng.integers(0, 4, (H, W))
    if not all_measured:
        z[bad & (kind == 0)] = 0.0
        z[bad & (kind == 1)] = -z[bad & (kind == 1)]
        z[bad & (kind == 2)] = np.inf
        z[bad & (kind == 3)] = np.nan
    I = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    T = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    same = rng.uniform(size=(H, W, 3)) < 0.10
    T[same] = I[same]
    return I, D, A, T, z


# ------------------------------------------------------------------------------------------------------------- SE(3)
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_exp_series(w, terms=30):
    """exp([w]x) by its power series in float64: independent of the tracker's closed form."""
    K = skew(np.asarray(w, np.float64))
    out, term = np.eye(3), np.eye(3)
    for k in range(1, terms):
        term = term @ K / k
        out = out + term
    return out


def pose_errors(rot, tran, rot_true, tran_true):
    """(|R - R_true|_F / sqrt 2 -- the rotation angle in radians for small angles --, |t - t_true|): the measures of
    tests/test_gpu_pose.py::test_pose_recovery."""
    return (float(np.linalg.norm(np.asarray(rot, np.float64) - np.asarray(rot_true, np.float64)) / math.sqrt(2.0)),
            float(np.linalg.norm(np.asarray(tran, np.float64) - np.asarray(tran_true, np.float64))))


def perturbed_start(rot_true, tran_true, seed=107, angle_deg=0.5, shift=0.02):
    """The start of test_pose_recovery: a rotation by ``angle_deg`` about a random axis in front of the true one, the
    translation ``shift`` off in a random direction (the same generator, the same draws)."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R0 = so3_exp_series(axis * math.radians(angle_deg)) @ np.asarray(rot_true, np.float64)
    sh = rng.normal(size=3)
    return R0, np.asarray(tran_true, np.float64) + sh / np.linalg.norm(sh) * shift
