"""Reference statements of gs_loss_track_gated (include/gs_abi.h) for tests/test_track_gate_host.py and
tests/test_gpu_track_gate.py -- a helper, not a test: the lower median by selection on the bit patterns, the sets, thresholds
and masks of the contract from a pair of residual maps, a float32 restatement of the residual maps, and the crafted inputs
whose residuals are exact."""
import numpy as np

from track_ref import measured

FLT_MAX = np.float32(3.402823466e38)


def in_set(resid):
    """resid <= FLT_MAX, false for NaN (and for +inf): the membership test of the contract."""
    resid = np.asarray(resid, np.float32)
    with np.errstate(invalid="ignore"):
        return resid <= FLT_MAX


def lower_median(values):
    """The element of rank (n - 1) // 2 of the non-negative float32 ``values`` in ascending order, 0 for an empty set -- by
    selection (np.partition) on the uint32 bit patterns, which order like the floats they encode; never an average."""
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    if v.size == 0:
        return np.float32(0)
    assert not np.signbit(v).any() and not np.isnan(v).any()
    k = (v.size - 1) // 2
    return np.partition(v.view(np.uint32), k)[k:k + 1].view(np.float32)[0]


def residuals_f32(I, D, A, T, z, alpha_min):
    """(a, c, covered, measured) as the contract states them in float32, one rounding per operation: c = (|d0| + |d1|) + |d2|
    on the covered pixels, a = |D / A - z| on the covered measured ones, NaN outside the sets.  (IEEE division and
    subtraction are correctly rounded: numpy's float32 gives the kernel's bits.)"""
    I, D, A, T = (np.asarray(x, np.float32) for x in (I, D, A, T))
    covered = A >= np.float32(alpha_min)
    meas = measured(z) if z is not None else np.zeros(A.shape, bool)
    d = np.abs(I - T)
    c = ((d[..., 0] + d[..., 1]) + d[..., 2]).astype(np.float32)
    rc = np.where(covered & in_set(c), c, np.float32(np.nan)).astype(np.float32)
    ra = np.full(A.shape, np.nan, np.float32)
    if z is not None:
        ok = covered & meas
        with np.errstate(all="ignore"):
            a = np.abs(np.where(ok, D, np.float32(1)) / np.where(ok, A, np.float32(1))
                       - np.where(ok, np.asarray(z, np.float32), np.float32(0))).astype(np.float32)
        ra = np.where(ok & in_set(a), a, np.float32(np.nan)).astype(np.float32)
    return ra, rc, covered, meas


def gate_from_residuals(ra, rc, covered, meas, k_d, k_c, floor_d=0.0, floor_c=0.0, couple=True):
    """The contract from the two residual maps (NaN outside the sets) -> dict: n_d, n_c, m_d, m_c, t_d, t_c (float32) and the
    masks ``dmask`` / ``cmask`` of the pixels whose depth / colour term counts."""
    ra, rc = np.asarray(ra, np.float32), np.asarray(rc, np.float32)
    s_d, s_c = in_set(ra), in_set(rc)
    m_d, m_c = lower_median(ra[s_d]), lower_median(rc[s_c])
    with np.errstate(invalid="ignore"):
        t_d = np.maximum(np.float32(k_d) * m_d, np.float32(floor_d))
        t_c = np.maximum(np.float32(k_c) * m_c, np.float32(floor_c))
        pass_d = s_d & (ra <= t_d)
        pass_c = s_c & (rc <= t_c)
    dmask = covered & meas & (pass_d if k_d > 0 else True)
    dropped = (s_d & ~pass_d) if (couple and k_d > 0) else np.zeros(ra.shape, bool)
    cmask = covered & ~dropped & (pass_c if k_c > 0 else True)
    return dict(n_d=int(s_d.sum()), n_c=int(s_c.sum()), m_d=np.float32(m_d), m_c=np.float32(m_c), t_d=np.float32(t_d),
                t_c=np.float32(t_c), dmask=dmask, cmask=cmask, s_d=s_d, s_c=s_c)


def crafted_inputs(H, W, resid, seed=5, covered=None, meas=None):
    """Inputs whose depth residuals are exactly ``resid`` ([H*W] or [H,W], >= 0): A = 1 and z = 1, D = 1 + resid, which the
    helper checks is exact in float32 both ways.  ``covered`` / ``meas`` (bool maps, default all): A = 0.25 where a pixel is
    not covered, z = 0 where it carries no measurement.  Image and target: uniform in [0, 1]."""
    r = np.asarray(resid, np.float32).reshape(H, W)
    D = (np.float32(1) + r).astype(np.float32)
    assert np.array_equal((D - np.float32(1)).astype(np.float32), r) and np.array_equal(D.astype(np.float64), 1.0 + r.astype(np.float64))
    A = np.ones((H, W), np.float32)
    z = np.ones((H, W), np.float32)
    if covered is not None:
        A[~np.asarray(covered, bool).reshape(H, W)] = 0.25
    if meas is not None:
        z[~np.asarray(meas, bool).reshape(H, W)] = 0.0
    rng = np.random.default_rng(seed)
    I = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    T = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    return I, D, A, T, z


def cycling(values, n, seed=7):
    """``n`` residuals that cycle through ``values``, shuffled."""
    v = np.asarray(values, np.float32)
    out = v[np.arange(n) % v.size]
    np.random.default_rng(seed).shuffle(out)
    return out


def powers_and_zeros(n):
    """2^-k for k = 1 .. 23 cycling, plus exact zeros: every residual in another level-0 bin, and the zero pattern."""
    return cycling(np.concatenate([2.0 ** -np.arange(1, 24), np.zeros(5)]), n)


def low_bits(n):
    """0.5 + j 2^-23, j = 0 .. 511 cycling: patterns that agree in their upper 22 bits and differ in the lowest ten only."""
    return cycling(0.5 + np.arange(512) * 2.0 ** -23, n)
