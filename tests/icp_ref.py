"""Reference statements of gs_icp_model_maps / gs_icp_step (include/gs_abi.h, csrc/icp_point.h) for tests/test_icp_host.py and
tests/test_gpu_icp.py -- a helper, not a test: the per-pixel rule in numpy, in float32 with one rounding per operation (the
kernels' vertices, normals and keep / drop decisions bit for bit) or in float64 (the algorithm alone), the 6 x 6 solve and the
pose update in float64, the whole staged alignment, and the analytic room corner the tests align against."""
import math

import numpy as np

from track_ref import so3_exp_series

N_TERMS = 28
STAGES = ((4, 4), (2, 5), (1, 10))


class Cam:
    """Size, focal lengths and the principal point's offset from the renderer's centre, as the kernels read a camera."""

    def __init__(self, width, height, focal_x, focal_y=None, dx=0.0, dy=0.0):
        self.width, self.height = int(width), int(height)
        self.focal_x = float(focal_x)
        self.focal_y = float(focal_x if focal_y is None else focal_y)
        self.dx, self.dy = float(dx), float(dy)


def origin(size):
    """left - padW / 2 of the frame path's padded image and centred crop (csrc/icp_point.h: gs_icp_origin)."""
    pad = (size + 15) // 16 * 16
    return (pad - size) // 2 - pad // 2


def measured(z):
    z = np.asarray(z)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


def rays(cam, dtype=np.float32):
    """(u [1,W], v [H,1], s [H,W]): the pixel centres' rays and their lengths, in the operation order of the kernels."""
    f = dtype
    un = (np.arange(cam.width, dtype=np.int64) + origin(cam.width)).astype(f) + f(0.5) - f(cam.dx)
    vn = (np.arange(cam.height, dtype=np.int64) + origin(cam.height)).astype(f) + f(0.5) - f(cam.dy)
    u = (un / f(cam.focal_x))[None, :]
    v = (vn / f(cam.focal_y))[:, None]
    s = np.sqrt(u * u + v * v + f(1.0))
    return u, v, s


def points(cam, z, dtype=np.float32):
    """[H,W,3]: the points at range z along the unit rays (garbage where z is no measurement)."""
    u, v, s = rays(cam, dtype)
    with np.errstate(all="ignore"):
        zc = np.asarray(z, dtype) / s
        return np.stack([u * zc, v * zc, zc], axis=-1).astype(dtype)


def model_range(depth, alpha, alpha_min, dtype=np.float32):
    """rho = D / A where A >= alpha_min (alpha given), else D; 0 where that is no measurement."""
    D = np.asarray(depth, dtype)
    with np.errstate(all="ignore"):
        if alpha is not None:
            A = np.asarray(alpha, dtype)
            rho = np.where(A >= dtype(alpha_min), D / A, dtype(0))
        else:
            rho = D
        return np.where(measured(rho), rho, dtype(0)).astype(dtype)


def model_maps(depth, alpha, cam, alpha_min=0.5, edge_rel=0.1, normal_step=1, dtype=np.float32):
    """(vertex [H,W,4], normal [H,W,4]) as gs_icp_model_maps writes them."""
    f = dtype
    H, W, s = cam.height, cam.width, int(normal_step)
    rho = model_range(depth, alpha, alpha_min, f)
    ok = rho != 0
    P = points(cam, rho, f)
    vertex = np.zeros((H, W, 4), f)
    vertex[..., :3] = np.where(ok[..., None], P, f(0))
    vertex[..., 3] = ok
    normal = np.zeros((H, W, 4), f)
    if H <= 2 * s or W <= 2 * s:
        return vertex, normal
    c = (slice(s, H - s), slice(s, W - s))
    xp, xm = (slice(s, H - s), slice(2 * s, W)), (slice(s, H - s), slice(0, W - 2 * s))
    yp, ym = (slice(2 * s, H), slice(s, W - s)), (slice(0, H - 2 * s), slice(s, W - s))
    five = [rho[c], rho[xp], rho[xm], rho[yp], rho[ym]]
    valid = ok[c] & ok[xp] & ok[xm] & ok[yp] & ok[ym]
    lo, hi = five[0], five[0]
    for r in five[1:]:
        lo, hi = np.minimum(lo, r), np.maximum(hi, r)
    if edge_rel >= 0:
        one_plus = f(1.0) + f(edge_rel)
        valid &= hi <= one_plus * lo
    with np.errstate(all="ignore"):
        a, b = P[xp] - P[xm], P[yp] - P[ym]
        c0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        c1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        c2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        l = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
        valid &= (l > 0) & np.isfinite(l)
        n = np.stack([c0 / l, c1 / l, c2 / l], axis=-1)
        v = P[c]
        flip = n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1] + n[..., 2] * v[..., 2] > 0
        n = np.where(flip[..., None], -n, n)
    inner = np.zeros(valid.shape + (4,), f)
    inner[..., :3] = np.where(valid[..., None], n, f(0))
    inner[..., 3] = valid
    normal[c] = inner
    return vertex, normal


def lattice(H, W, stride):
    off = stride // 2
    return np.arange(off, H, stride), np.arange(off, W, stride)


def step_terms(range_map, cam, vertex, normal, mcam, R, t, stride, dist_max, cos_min, dtype=np.float32):
    """One accumulation pass -> (terms [kept, 28] in ``dtype`` in row-major lattice order, kept, measured lattice pixels).
    (R, t): the float64 state, rounded to ``dtype`` once."""
    f = dtype
    ys, xs = lattice(cam.height, cam.width, int(stride))
    z = np.asarray(range_map, f)[np.ix_(ys, xs)]
    has = measured(z)
    P = points(cam, range_map, f)[np.ix_(ys, xs)]
    Rf, tf = np.asarray(R, np.float64).reshape(3, 3).astype(f), np.asarray(t, np.float64).reshape(3).astype(f)
    with np.errstate(all="ignore"):
        q = [Rf[i, 0] * P[..., 0] + Rf[i, 1] * P[..., 1] + Rf[i, 2] * P[..., 2] + tf[i] for i in range(3)]
        fx = f(mcam.focal_x) * (q[0] / q[2]) + f(mcam.dx) - f(origin(mcam.width))
        fy = f(mcam.focal_y) * (q[1] / q[2]) + f(mcam.dy) - f(origin(mcam.height))
        keep = has & (q[2] > 0) & (fx >= 0) & (fx < f(mcam.width)) & (fy >= 0) & (fy < f(mcam.height))
        i = np.where(keep, np.floor(fx), 0).astype(np.int64)
        j = np.where(keep, np.floor(fy), 0).astype(np.int64)
        V, Nm = np.asarray(vertex, f)[j, i], np.asarray(normal, f)[j, i]
        keep &= Nm[..., 3] != 0
        d = [q[k] - V[..., k] for k in range(3)]
        keep &= d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= f(dist_max) * f(dist_max)
        nv = Nm[..., 0] * V[..., 0] + Nm[..., 1] * V[..., 1] + Nm[..., 2] * V[..., 2]
        keep &= -nv >= f(cos_min) * np.sqrt(V[..., 0] * V[..., 0] + V[..., 1] * V[..., 1] + V[..., 2] * V[..., 2])
        n = [Nm[..., k] for k in range(3)]
        e = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
        J = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]]
        cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * e for a in range(6)] + [e * e]
    terms = np.stack([c[keep] for c in cols], axis=-1).astype(f)
    return terms, int(keep.sum()), int(has.sum())


def unpack(sums):
    """The 28 sums -> (A [6,6] symmetric, b [6], sum e e)."""
    sums = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = sums[k]
            k += 1
    return A, sums[21:27].copy(), float(sums[27])


def solve(A, b, damping):
    """x of (A + damping tr(A) / 6 I) x = -b in float64, and that lambda; None when the matrix is not positive definite."""
    lam = float(damping) * float(np.trace(A)) / 6.0
    M = A + lam * np.eye(6)
    try:
        np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None, lam
    return np.linalg.solve(M, -b), lam


def update(R, t, x):
    """R <- exp([x_w]x) R, t <- exp([x_w]x) t + x_t in float64."""
    E = so3_exp_series(x[:3])
    return E @ np.asarray(R, np.float64).reshape(3, 3), E @ np.asarray(t, np.float64).reshape(3) + x[3:]


def align(range_map, cam, vertex, normal, mcam, R, t, stages=STAGES, dist_max=0.2, cos_min=0.0, damping=1e-6, min_count=6,
          dtype=np.float64):
    """The staged alignment -> (R, t, rows): rows = per iteration (kept, measured, rmse, status 0 / 1 / 2)."""
    R, t = np.asarray(R, np.float64).reshape(3, 3).copy(), np.asarray(t, np.float64).reshape(3).copy()
    rows = []
    for stride, n in stages:
        for _ in range(n):
            terms, kept, meas = step_terms(range_map, cam, vertex, normal, mcam, R, t, stride, dist_max, cos_min, dtype)
            A, b, ee = unpack(terms.astype(np.float64).sum(axis=0))
            status, x = 0, None
            if kept < min_count:
                status = 1
            else:
                x, _ = solve(A, b, damping)
                status = 0 if x is not None else 2
            if status == 0:
                R, t = update(R, t, x)
            rows.append((kept, meas, math.sqrt(ee / kept) if kept else 0.0, status))
    return R, t, rows


# ------------------------------------------------------------------------------------------------------- pose algebra
def relative(rot_m, tran_m, rot_f, tran_f):
    """(R, t) with p_model = R p_frame + t for two world -> camera poses, in float64."""
    R = np.asarray(rot_m, np.float64) @ np.asarray(rot_f, np.float64).T
    return R, np.asarray(tran_m, np.float64) - R @ np.asarray(tran_f, np.float64)


def frame_pose(rot_m, tran_m, R, t):
    """The frame's world -> camera pose from the model's and (R, t): rot = R^T rot_m, tran = R^T (tran_m - t)."""
    return R.T @ np.asarray(rot_m, np.float64), R.T @ (np.asarray(tran_m, np.float64) - t)


# ------------------------------------------------------------------------------------------------------- the corner
CORNER_W, CORNER_H, CORNER_F = 160, 120, 120.0
CORNER_PLANES = ((0, -1.2), (1, 1.0), (2, 3.0))  # world planes x = -1.2, y = 1.0, z = 3.0, seen from inside
CORNER_ROT = so3_exp_series(np.array([0.05, 0.35, 0.02]))
CORNER_TRAN = np.array([0.1, -0.05, 0.2])
SLIDING_ROT = so3_exp_series(np.array([0.05, -0.35, 0.02]))  # the plane x = -1.2 leaves the view
STARTS = ((0.5, 0.02), (2.0, 0.08), (4.0, 0.16))


def corner_camera():
    return Cam(CORNER_W, CORNER_H, CORNER_F)


def corner_range(rot, tran, cam=None, planes=CORNER_PLANES, with_index=False):
    """The exact range map of the corner from the world -> camera pose (rot, tran): the nearest positive ray-plane hit along
    each pixel's unit ray, in float64 (0 where there is none)."""
    cam = cam or corner_camera()
    rot, tran = np.asarray(rot, np.float64).reshape(3, 3), np.asarray(tran, np.float64).reshape(3)
    u, v, s = rays(cam, np.float64)
    d_cam = np.stack([u / s, v / s, 1.0 / s], axis=-1)  # unit rays in the camera's frame
    d = d_cam @ rot                                    # rot^T d, per pixel
    o = -rot.T @ tran
    best = np.full(d.shape[:2], np.inf)
    index = np.full(d.shape[:2], -1)
    for k, (axis, c) in enumerate(planes):
        with np.errstate(divide="ignore", invalid="ignore"):
            hit = (c - o[axis]) / d[..., axis]
        better = (hit > 0) & (hit < best)
        best = np.where(better, hit, best)
        index = np.where(better, k, index)
    rng = np.where(np.isfinite(best), best, 0.0)
    return (rng, index) if with_index else rng


def seeded_start(rot_true, tran_true, seed, angle_deg, shift):
    """track_ref.perturbed_start's construction with a seeded axis."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R0 = so3_exp_series(axis * math.radians(angle_deg)) @ np.asarray(rot_true, np.float64)
    sh = rng.normal(size=3)
    return R0, np.asarray(tran_true, np.float64) + sh / np.linalg.norm(sh) * shift



# ------------------------------------------------------------------------------------------------- inputs of the tests
MAP_SIZES = ((7, 9), (48, 64), (120, 160), (187, 250))  # H x W
PP_OFFSET = (7.3, -4.6)
ALPHA_MIN, EDGE_REL = 0.5, 0.1


def maps_case(H, W, seed, pp=(0.0, 0.0)):
    """Inputs of the model-map test: a smooth range map with a depth step of 1.5 x across a slanted line (the edge rule decides
    there), holes of every kind of "no measurement" (the border of a hole decides like the image border), and alpha in
    [0.3, 1] straddling alpha_min = 0.5 with D = fl(rho A).  -> (cam, D, A, rho)."""
    rng = np.random.default_rng(seed)
    cam = Cam(W, H, 0.75 * W, 0.8 * W, *pp)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rho = 2.0 + 0.3 * np.sin(x / 7.0) + 0.2 * np.cos(y / 5.0)
    rho = np.where(x + 0.5 * y > 0.6 * W, 1.5 * rho, rho).astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.06
    kind = rng.integers(0, 4, (H, W))
    rho[bad & (kind == 0)] = 0.0
    rho[bad & (kind == 1)] = -rho[bad & (kind == 1)]
    rho[bad & (kind == 2)] = np.inf
    rho[bad & (kind == 3)] = np.nan
    A = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        D = (rho * A).astype(np.float32)
    return cam, D, A, rho


def step_case(H, W, seed, model_size=None, model_pp=(0.0, 0.0), frame_pp=(0.0, 0.0)):
    """Inputs of the step test: the room corner seen by a frame camera H x W at the true pose and by the model camera (the same
    size unless ``model_size`` = (Hm, Wm)) 2 degrees / 0.08 off; 3 % of the frame's ranges carry no measurement; the state is
    1 degree / 0.03 off the identity.  -> dict(cam, mcam, z, zm, R, t)."""
    rng = np.random.default_rng(seed)
    Hm, Wm = model_size or (H, W)
    cam, mcam = Cam(W, H, 0.75 * W, None, *frame_pp), Cam(Wm, Hm, 0.75 * Wm, None, *model_pp)
    rot_m, tran_m = seeded_start(CORNER_ROT, CORNER_TRAN, seed, 2.0, 0.08)
    z = corner_range(CORNER_ROT, CORNER_TRAN, cam).astype(np.float32)
    zm = corner_range(rot_m, tran_m, mcam).astype(np.float32)
    bad = rng.uniform(size=(H, W)) < 0.03
    kind = rng.integers(0, 4, (H, W))
    z[bad & (kind == 0)] = 0.0
    z[bad & (kind == 1)] = -1.0
    z[bad & (kind == 2)] = np.inf
    z[bad & (kind == 3)] = np.nan
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    R = so3_exp_series(axis * math.radians(1.0))
    t = rng.normal(size=3)
    t = t / np.linalg.norm(t) * 0.03
    return dict(cam=cam, mcam=mcam, z=z, zm=zm, R=R, t=t, rot_m=rot_m, tran_m=tran_m)
