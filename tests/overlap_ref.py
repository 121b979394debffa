"""NumPy restatements of the covisibility count (include/gs_abi.h, gs_view_overlap; csrc/overlap_point.h), for the tests.

``counts_f32``: the contract in float32, operation by operation, one rounding each -- it must decide every point exactly as
the kernel does.  ``counts_f64``: the same geometry in float64 from the same float32 inputs, with a per-view mask of the
points float32 cannot be expected to decide: a border inequality within a relative 1e-5 of |q.z| W_k of flipping, or q.z
within a relative 1e-5 of ``near``.  ``cases()`` builds the inputs: the smallest shapes at which the kernel can go wrong.
``plan`` restates the launch plan; ``LONG_CASES``, ``GROUP_EDGE_CASES`` and ``band_case`` are the inputs beyond its thresholds
(tests/test_gpu_slam_regimes.py)."""
import math
from types import SimpleNamespace

import numpy as np

from seed_ref import lattice

F = np.float32
UND_REL = 1e-5


def origin(size):
    """left - padW / 2 of the padded image and centred crop: minus the `cx` of the contract."""
    pad = (int(size) + 15) // 16 * 16
    return (pad - int(size)) // 2 - pad // 2


def measured_lattice(z, stride):
    """(ys, xs, ranges) of the measured lattice pixels (z > 0 and finite) in row-major order."""
    z = np.asarray(z, F)
    ys, xs = lattice(z.shape[0], z.shape[1], stride)
    r = z[ys, xs]
    with np.errstate(invalid="ignore"):
        m = (r > F(0)) & (r <= np.finfo(F).max)
    return ys[m], xs[m], r[m]


def _cam_arrays(cam, dtype):
    rot = np.asarray(cam.rot, F).astype(dtype).reshape(9)
    tran = np.asarray(cam.tran, F).astype(dtype).reshape(3)
    return rot, tran, dtype(F(cam.focal_x)), dtype(F(cam.focal_y))


def points(z, cam, stride, dtype=F):
    """(ys, xs, p [3][n]) of the measured lattice pixels: the world point gs_seed_apply writes, in its operation order."""
    ys, xs, r = measured_lattice(z, stride)
    rot, tran, fx, fy = _cam_arrays(cam, dtype)
    r = r.astype(dtype)
    u = ((xs + origin(cam.width)).astype(dtype) + dtype(0.5)) / fx
    v = ((ys + origin(cam.height)).astype(dtype) + dtype(0.5)) / fy
    zc = r / np.sqrt(u * u + v * v + dtype(1.0))
    q0, q1, q2 = u * zc - tran[0], v * zc - tran[1], zc - tran[2]
    p = [rot[k] * q0 + rot[3 + k] * q1 + rot[6 + k] * q2 for k in range(3)]
    return ys, xs, p


def _view_terms(p, view, border, dtype):
    """q.z and the four (lhs, rhs) pairs of the border tests of one view, in the contract's operation order."""
    rot, tran, fx, fy = _cam_arrays(view, dtype)
    qx = rot[0] * p[0] + rot[1] * p[1] + rot[2] * p[2] + tran[0]
    qy = rot[3] * p[0] + rot[4] * p[1] + rot[5] * p[2] + tran[1]
    qz = rot[6] * p[0] + rot[7] * p[1] + rot[8] * p[2] + tran[2]
    ox, oy = origin(view.width), origin(view.height)
    ax, ay = fx * qx, fy * qy
    lo_x, hi_x = dtype(border + ox) * qz, dtype(int(view.width) - border + ox) * qz
    lo_y, hi_y = dtype(border + oy) * qz, dtype(int(view.height) - border + oy) * qz
    return qz, ((ax, lo_x, True), (ax, hi_x, False), (ay, lo_y, True), (ay, hi_y, False))


def seen_f32(z, cam, views, stride, near, border):
    """bool [n_views, measured lattice pixels]: the float32 decisions."""
    _, _, p = points(z, cam, stride, F)
    out = np.zeros((len(views), len(p[0])), bool)
    for k, view in enumerate(views):
        qz, tests = _view_terms(p, view, border, F)
        s = qz > F(near)
        for lhs, rhs, ge in tests:
            s &= (lhs >= rhs) if ge else (lhs < rhs)
        out[k] = s
    return out


def _counts(seen):
    n_views, n = seen.shape
    c = np.zeros(n_views + 2, np.int64)
    c[:n_views] = seen.sum(1)
    c[n_views] = n
    c[n_views + 1] = n - int(seen.any(0).sum())
    return c


def counts_f32(z, cam, views, stride, near, border):
    return _counts(seen_f32(z, cam, views, stride, near, border))


def counts_f64(z, cam, views, stride, near, border):
    """-> (counts [n_views + 2] int64, undecidable bool [n_views, n]).  A point is undecidable for a view when a test that
    float32 may decide either way can change the outcome: every decidable test passes and at least one is not decidable."""
    _, _, p = points(z, cam, stride, np.float64)
    n_views, n = len(views), len(p[0])
    seen, und = np.zeros((n_views, n), bool), np.zeros((n_views, n), bool)
    near = float(F(near))
    for k, view in enumerate(views):
        qz, tests = _view_terms(p, view, border, np.float64)
        ok = qz > near
        soft = np.abs(qz - near) <= UND_REL * near
        passes, softs = [ok], [soft]
        for lhs, rhs, ge in tests:
            passes.append((lhs >= rhs) if ge else (lhs < rhs))
            softs.append(np.abs(lhs - rhs) <= UND_REL * np.abs(qz) * float(view.width))
        seen[k] = np.logical_and.reduce(passes)
        und[k] = np.logical_and.reduce([a | b for a, b in zip(passes, softs)]) & np.logical_or.reduce(softs)
    return _counts(seen), und


# ------------------------------------------------------------------------------------------------------------ the cases
def _roty(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])


def _rotx(deg):
    a = math.radians(deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])


def _camera(W, H, fx, fy, rot, tran):
    return SimpleNamespace(width=int(W), height=int(H), focal_x=float(F(fx)), focal_y=float(F(fy)),
                           rot=np.asarray(rot, np.float64).astype(F).reshape(3, 3), tran=np.asarray(tran, np.float64).astype(F),
                           near=0.3)


def _moved(cam, dR, dt, W=None, H=None, fx=None, fy=None):
    """The camera whose frame is cam's moved by (dR, dt): q = dR (rot p + tran) + dt."""
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    return _camera(W or cam.width, H or cam.height, fx or cam.focal_x, fy or cam.focal_y, dR @ R, dR @ t + np.asarray(dt))


def range_map(H, W, seed):
    """A smooth surface plus steps, about 10 % of the pixels without a measurement: zeros, negatives, inf and NaN."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 2.5 + 0.8 * np.sin(xs / 9.0) * np.cos(ys / 7.0) + 1.0 * (xs > 0.6 * W) - 0.7 * (ys > 0.7 * H)
    z = z.astype(F)
    kind = rng.integers(0, 40, (H, W))
    z[kind == 0] = 0.0
    z[kind == 1] = -1.5
    z[kind == 2] = np.inf
    z[kind == 3] = np.nan
    return z


BAND_ROWS = (51, 200, 201, 400, 401, 402, -1)  # lattice rows (-1: the last one, which the ragged last chunk ends)


def range_map_bands(H, W, stride, seed):
    """range_map with whole lattice rows unmeasured -- 0, NaN, -1 and inf cycling along the row -- in bands of one, two and
    three rows and in the last row: runs of more than 256 lattice pixels in a row without a measurement, which the scattered
    10 % of range_map never give.  (A row of every LONG_SHAPES lattice is at least 724 pixels long.)"""
    z = range_map(H, W, seed)
    off = stride // 2
    rows = np.arange(off, H, stride)
    blank = np.array([0.0, np.nan, -1.0, np.inf], F)[np.arange(W) % 4]
    for ly in BAND_ROWS:
        z[rows[ly]] = np.roll(blank, ly)
    return z


def skip_situations(z, stride):
    """-> three arrays of workgroup numbers under plan(): first chunk blank and a later one measured; first chunk measured
    and a later (existing) one blank; every chunk blank."""
    _, chunks, per, nblk = plan(z.shape[0], z.shape[1], stride)
    m = chunk_measured(z, stride)
    assert len(m) == chunks
    exists = (np.arange(nblk * per) < chunks).reshape(nblk, per)
    m = np.concatenate([m, np.zeros(nblk * per - chunks, bool)]).reshape(nblk, per)
    return (np.flatnonzero(~m[:, 0] & m[:, 1:].any(1)), np.flatnonzero(m[:, 0] & (~m[:, 1:] & exists[:, 1:]).any(1)),
            np.flatnonzero(~m.any(1)))


def chunk_measured(z, stride):
    """bool [chunks]: does chunk c -- lattice pixels [256 c, 256 c + 256) in row-major order -- hold a measurement?"""
    z = np.asarray(z, F)
    ys, xs = lattice(z.shape[0], z.shape[1], stride)
    r = z[ys, xs]
    with np.errstate(invalid="ignore"):
        m = (r > F(0)) & (r <= np.finfo(F).max)
    pad = -len(m) % OVL_BLOCK
    return np.concatenate([m, np.zeros(pad, bool)]).reshape(-1, OVL_BLOCK).any(1)


SHAPES = ((37, 53, 1), (120, 160, 2), (64, 64, 3))  # (37, 53): padded 48 x 64, crop left = top = 5, 1,961 lattice pixels
N_VIEWS = (1, 3, 65, 256)
NEAR = 0.3
SPECIAL = ("own", "behind", "other size and focal", "sideways", "yawed", "forward")
# seeds of the random views, chosen on the CPU so that no view has more undecidable points than 0.1 % of the measured ones
# (tests/test_overlap_host.py asserts it): with 394 measured points that means none at all
VIEW_SEEDS = {(64, 65): 1, (64, 256): 80, (37, 128): 2, (37, 192): 1, (37, 193): 2}
_CACHE = {}

# csrc/overlap.hip: `constexpr int OVL_BLOCK = 256` lattice pixels to a chunk, `constexpr int OVL_MAX_BLOCKS = 2048` workgroups
OVL_BLOCK, OVL_MAX_BLOCKS = 256, 2048
# The smallest shapes whose workgroups run over more than one chunk (plan(); tests/test_gpu_slam_regimes.py):
#   (725, 724, 1)  : 524,900 lattice pixels, 2,051 chunks, 2 per workgroup, 1,026 workgroups; the last one holds one ragged chunk
#   (1449, 1450, 2): the same plan through a stride-2 lattice with offset 1
#   (1025, 1024, 1): 4,100 chunks, 3 per workgroup, 1,367 workgroups; the last one holds two of its three
LONG_SHAPES = ((725, 724, 1), (1449, 1450, 2), (1025, 1024, 1))
LONG_CASES = tuple((H, W, s, 7) for H, W, s in LONG_SHAPES) + ((725, 724, 1, 65),)
# the edges of the kernel's view groups (`kend = min(64, n_views - 64 * g)`), on the smallest shape
GROUP_EDGE_CASES = tuple((37, 53, 1, n) for n in (64, 128, 129, 192, 193))


def plan(H, W, stride):
    """-> (L, chunks, chunks_per_block, nblk): overlap_plan of csrc/overlap.hip, restated."""
    off = stride // 2
    Lw = (W - off + stride - 1) // stride if W > off else 0
    Lh = (H - off + stride - 1) // stride if H > off else 0
    L = Lw * Lh
    chunks = -(-L // OVL_BLOCK)
    per = -(-chunks // OVL_MAX_BLOCKS) if chunks > OVL_MAX_BLOCKS else 1
    return L, chunks, per, -(-chunks // per)


def case(H, W, stride, n_views):
    """-> dict(z, cam, views, stride, near): computed once per case, never modified.  The views start with SPECIAL, in that
    order: the frame's own camera; one turned 180 degrees about y (sees nothing); one of another size and focal length;
    one moved sideways; one yawed; one moved forward past part of the surface (points fall behind `near`); the rest are
    small random motions."""
    key = (H, W, stride, n_views)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * H + 10 * stride + n_views + 100000 * VIEW_SEEDS.get((H, n_views), 0))
        cam = _camera(W, H, 0.75 * W, 0.8 * W, _roty(2.0) @ _rotx(-1.0), [0.03, -0.01, 0.2])
        I = np.eye(3)
        views = [_moved(cam, I, [0, 0, 0]), _moved(cam, _roty(180.0), [0, 0, 0]),
                 _moved(cam, _rotx(3.0), [0.1, 0.05, 0.3], W=W + 11, H=H + 6, fx=0.6 * W, fy=0.9 * W),
                 _moved(cam, I, [0.9, 0.0, 0.0]), _moved(cam, _roty(14.0), [0.0, 0.1, 0.0]),
                 _moved(cam, I, [0.0, 0.0, -2.2])]
        while len(views) < n_views:
            a = rng.uniform(-12.0, 12.0, 2)
            views.append(_moved(cam, _roty(a[0]) @ _rotx(a[1]), rng.uniform(-0.5, 0.5, 3)))
        _CACHE[key] = dict(z=range_map(H, W, seed=H + W + stride), cam=cam, views=views[:n_views], stride=stride, near=NEAR)
    return _CACHE[key]


def cases():
    return [(H, W, s, n) for H, W, s in SHAPES for n in N_VIEWS]


def band_case(H, W, stride, n_views):
    """case() with the range map of range_map_bands (the same seed): computed once, never modified."""
    key = (H, W, stride, n_views, "bands")
    if key not in _CACHE:
        _CACHE[key] = dict(case(H, W, stride, n_views), z=range_map_bands(H, W, stride, seed=H + W + stride))
    return _CACHE[key]


_REFERENCE = {}


def reference(H, W, stride, n_views, border):
    """-> dict(c32, c64, und_per_view, und_any) of case(H, W, stride, n_views): both restatements, evaluated once per process
    (seconds each at LONG_SHAPES) and shared by the tests that need them."""
    key = (H, W, stride, n_views, border)
    if key not in _REFERENCE:
        k = case(H, W, stride, n_views)
        c64, und = counts_f64(k["z"], k["cam"], k["views"], stride, k["near"], border)
        _REFERENCE[key] = dict(c32=counts_f32(k["z"], k["cam"], k["views"], stride, k["near"], border), c64=c64,
                               und_per_view=und.sum(1), und_any=int(und.any(0).sum()))
    return _REFERENCE[key]


def table_rows(views):
    """float32 [n, 16]: the views as gs_seed_camera rows (width and height as their int32 bit patterns)."""
    rows = np.zeros((len(views), 16), F)
    for k, v in enumerate(views):
        rows[k, :9], rows[k, 9:12] = np.asarray(v.rot, F).reshape(9), np.asarray(v.tran, F)
        rows[k, 12], rows[k, 13] = F(v.focal_x), F(v.focal_y)
        rows[k, 14:16] = np.array([v.width, v.height], np.int32).view(F)
    return rows


def own_view_count(z, stride, border):
    """Closed form for the frame's own camera: every measured lattice pixel falls back on its own pixel centre, so the count
    is the measured lattice pixels inside the window shrunk by `border`."""
    ys, xs, _ = measured_lattice(z, stride)
    H, W = np.asarray(z).shape
    return int(((xs >= border) & (xs < W - border) & (ys >= border) & (ys < H - border)).sum())
