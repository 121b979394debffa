"""The float32 restatement of gs_pyramid_down (include/gs_abi.h; csrc/pyramid.hip) in numpy: the contract's expressions in
their order, every operation on float32 arrays (one rounding per operation), plus the inputs the two test tiers share."""
import numpy as np

F = np.float32


def measured(z):
    """> 0 and finite: the rule of gs_loss_depth / gs_loss_track."""
    return (z > 0) & np.isfinite(z)


def down(image, rng=None, min_valid=2, edge_rel=0.1):
    """(image_out [H/2,W/2,3], range_out [H/2,W/2] or None).  image [H,W,3] and rng [H,W] float32, H and W even."""
    image = np.asarray(image, F)
    a00, a01, a10, a11 = image[0::2, 0::2], image[0::2, 1::2], image[1::2, 0::2], image[1::2, 1::2]
    with np.errstate(all="ignore"):
        out = (((a00 + a01) + a10) + a11) * F(0.25)
        assert out.dtype == F
        if rng is None:
            return out, None
        rng = np.asarray(rng, F)
        z = [rng[0::2, 0::2], rng[0::2, 1::2], rng[1::2, 0::2], rng[1::2, 1::2]]
        m = [measured(v) for v in z]
        v = [np.where(mk, zk, F(0.0)).astype(F) for mk, zk in zip(m, z)]
        n = m[0].astype(np.int32) + m[1] + m[2] + m[3]
        lo = np.full(n.shape, np.inf, F)
        hi = np.zeros(n.shape, F)
        for mk, vk in zip(m, v):
            lo = np.where(mk, np.minimum(lo, vk), lo)
            hi = np.where(mk, np.maximum(hi, vk), hi)
        s = ((v[0] + v[1]) + v[2]) + v[3]
        one_plus = F(F(1.0) + F(edge_rel))
        ok = n >= min_valid
        if not F(edge_rel) < 0:
            ok = ok & (hi <= one_plus * lo)
        val = s / np.maximum(n, 1).astype(F)
        assert s.dtype == F and val.dtype == F and (one_plus * lo).dtype == F
        return out, np.where(ok, val, F(0.0)).astype(F)


def level(image, rng, l, min_valid=2, edge_rel=0.1):
    """Level l of a pyramid: ``down`` applied l times."""
    for _ in range(l):
        image, rng = down(image, rng, min_valid, edge_rel)
    return image, rng


def next_up(x):
    return np.nextafter(F(x), F(np.inf))


def inputs(H, W, seed):
    """(image [H,W,3], range [H,W]) float32.  The range map mixes measured values (1 .. 5, smooth plus steps, so that the
    0.1 edge test both passes and fails) with 0, negatives, NaN and +-inf; the first footprints are crafted:
      (0, 0..4): n = 0, 1, 2, 3, 4 measured, equal values (whenever the map is wide enough: 2 columns per footprint);
      row 1 (footprints (1, 0) and (1, 1), when present): lo = 2, hi exactly fl(fl(1.1f) 2) -- counts at edge_rel 0.1 --
      and the next float above it -- does not."""
    r = np.random.default_rng(seed)
    image = r.uniform(0.0, 1.0, (H, W, 3)).astype(F)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (2.0 + 0.3 * np.sin(xx / 5.0) + 0.2 * np.cos(yy / 3.0) + 1.5 * ((xx // 3 + yy // 5) % 3 == 0)).astype(F)
    z *= r.uniform(0.97, 1.03, (H, W)).astype(F)
    kind = r.integers(0, 20, (H, W))
    z[kind == 0] = 0.0
    z[kind == 1] = -1.5
    z[kind == 2] = np.nan
    z[kind == 3] = np.inf
    z[kind == 4] = -np.inf
    bad = [0.0, np.nan, -2.0, np.inf]
    for j in range(min(5, W // 2)):  # footprint (0, j): j measured pixels of value 3
        cells = [(0, 2 * j), (0, 2 * j + 1), (1, 2 * j), (1, 2 * j + 1)]
        for k, (y, x) in enumerate(cells):
            z[y, x] = 3.0 if k < j else bad[k]
    if H >= 4:
        top = F(F(1.0) + F(0.1)) * F(2.0)
        z[2:4, 0:2] = [[2.0, top], [2.05, 2.1]]
        if W >= 4:
            z[2:4, 2:4] = [[2.0, next_up(top)], [2.05, 2.1]]
    return image, z.astype(F)
