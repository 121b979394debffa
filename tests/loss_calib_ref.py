"""Inputs, truth and conditioning for the calibration of the L1 + SSIM loss gradient (gs_loss_l1_ssim, gs_loss_l1_ssim_weighted)
-- a helper of tests/test_loss_calibration_host.py and tests/test_gpu_loss_calibration.py, not a test; numpy only.

* ``pairs(H, W)``     the image pairs training sees: flat black / white backgrounds, a prediction that is all background, one that
                      is almost the target, one that IS the target, constants, a flat half next to noise, exact ties.
* ``weight_maps``     all ones, a zero-weight blob touching a border (what gs_track_gate_mask produces), soft weights with the blob.
* ``evaluate``        oracle.train_ref.l1_ssim_loss / gate_map_ref.weighted_l1_ssim_loss on the fp32 inputs: the truth at float64, the
                      reference arithmetic at float32.
* ``scale``           per gradient element, the sum of magnitudes the element is built from (the rule of gs_testutil.grad_close):
                      an evaluation in a format of unit roundoff u errs by (a small count of operations) x u x scale, whatever its
                      order of operations.  F_REF below is that count as measured for the numpy-float32 restatement.

How ``scale`` is built.  With M_q = (mu, nu, Exx, Eyy, Exy) the moments of window q and (dmu, dExx, dExy)_q the three partial
derivatives of S there, the gradient is

    grad_p = a m_p sign(x_p - y_p) - b sum_q g(p - q) m_q G_pq,   G_pq = dmu_q + 2 x_p dExx_q + y_p dExy_q
           = (T1 - T2)_q + 2 (x_p - mu_q) dExx_q + y_p dExy_q     (dmu = T1 - T2 - 2 mu dExx).

Every evaluation -- numpy, the kernels -- computes the intermediates of a window ONCE and feeds them to all three adjoints, so an
error of an intermediate s of window q reaches grad_p as b g(p - q) m_q (dG_pq / ds) ds: the derivative of the whole bracket, not
the sum of the magnitudes of its parts.  (On a flat background that is the difference between a scale of 10^3 b and one of 10^7 b:
dExx alone moves by S E[B2] / B2^2, but it enters as 2 (x_p - mu_q) dExx and x_p = mu_q there.)  The sources s and their
magnitudes per unit roundoff:

    mu, nu     the filter sums, g*|x| and g*|y|; their derivative is the total one, through A1, A2, B1, B2 and the explicit factors
    A1         |A1| + 2 |mu nu|
    A2         |A2| + 2 (|Exy| + |mu nu| + g*|x y|)                            -- the cancellation Exy - mu nu
    B1         B1 + mu^2 + nu^2
    B2         B2 + (Exx + mu^2 + g*x^2) + (Eyy + nu^2 + g*y^2)               -- the cancellations Exx - mu^2 and Eyy - nu^2

each weighted by |dG_pq / ds| = |alpha_s + beta_s (x_p - mu_q) + gamma_s y_p|, summed over the windows q that reach p (``_reach``),
plus the last roundings of T1, T2, 2 mu dExx, dExx and dExy and of the adjoint filters, as plain magnitudes.

The clamp.  dExx = (vx_raw > 0 ? -S / B2 : 0) is discontinuous, and where the variance is exactly zero the decision falls on
rounding noise -- in float64 as in float32.  There 2 (x_p - mu_q) dExx is rounding noise whichever way it goes, so dExx counts as
-S / B2 whatever the clamp decided, and in a window whose |vx_raw| lies within AMBIGUOUS x u x its magnitude (a) the part of each
derivative that runs through dExx or through dB2/dmu is added in magnitude, not in sign, so that either decision is bounded, and
(b) the difference 2 g |x_p - mu_q| S / B2 between the two decisions is added whole.
"""
import numpy as np

from gate_map_ref import weighted_l1_ssim_loss
from oracle.train_ref import _filt_full_adjoint, _filt_valid, gaussian_window, l1_ssim_loss

U = 2.0 ** -24  # unit roundoff of fp32

# The numpy-float32 restatement's worst |g32 - g64| / (U scale) over HOST_CASES and the same for the SSIM value, as
# tests/test_loss_calibration_host.py measures them (3.63 and 0.673, profiles/loss_calibration.txt), recorded with headroom.  The
# gradient's figure is set by elements a full window away from the nearest non-zero pixel, which see the image through the
# outermost tap alone: in fp32 that tap of the window is 4.4 ulp off (its exponent, -50 / 9, amplifies the rounding of the
# argument), it enters four times, and one more ulp of exp there would move the figure by 0.75.  Everywhere else the restatement
# stays below 1.1.  The GPU test grants the kernels 8 x these.
F_REF = 4.5
F_REF_SSIM = 0.75

AMBIGUOUS = 64.0  # >= 8 F_REF: a clamp decision that an evaluation within the asserted bound may take either way

PAIR_NAMES = ("noise", "black_bg", "white_bg", "late_fit", "equal", "const", "half_flat", "ties")
WEIGHT_NAMES = ("ones", "blob", "soft")
DISC_COLOUR = (0.9, 0.5, 0.2)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _discs(H, W):
    """(mask [H, W], colours [H, W, 3]) of a lattice of discs, 34 rows and 38 columns apart around a point off the centre, radius
    a quarter of the short side but 9 at most (and one pixel at least); the colour rotates from disc to disc.  The gaps leave
    background that no window through a disc reaches, and no 52-row or 160-pixel boundary of a kernel lies further than that reach
    from a disc's edge once the image is large enough to have one."""
    cy, cx, r = 0.45 * H, 0.55 * W, min(max(0.25 * min(H, W), 1.0), 9.0)
    yy, xx = np.mgrid[0:H, 0:W]
    iy, ix = np.rint((yy - cy) / 34.0), np.rint((xx - cx) / 38.0)
    mask = (yy - cy - 34.0 * iy) ** 2 + (xx - cx - 38.0 * ix) ** 2 <= r * r
    turn = ((iy + ix).astype(int) % 3)[:, :, None]
    base = np.asarray(DISC_COLOUR, np.float32)
    colours = np.where(turn == 0, base, np.where(turn == 1, np.roll(base, 1), np.roll(base, 2)))
    return mask, colours.astype(np.float32)


def _box_blur(a, passes):
    """3 x 3 box blur with replicated edges in float64: a constant region stays that constant exactly ((c + c + c) / 3 = c)."""
    a = np.asarray(a, np.float64)
    for _ in range(passes):
        p = np.pad(a, ((1, 1), (0, 0), (0, 0)), mode="edge")
        a = (p[:-2] + p[1:-1] + p[2:]) / 3.0
        p = np.pad(a, ((0, 0), (1, 1), (0, 0)), mode="edge")
        a = (p[:, :-2] + p[:, 1:-1] + p[:, 2:]) / 3.0
    return a


def pairs(H, W):
    """{name: (pred, target)} of float32 [H, W, 3] images, a deterministic function of (H, W)."""
    rng = np.random.default_rng(H * 1000 + W)
    disc, colour = _discs(H, W)
    out = {}
    x = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1).astype(np.float32)
    y[::7, ::5] = x[::7, ::5]
    out["noise"] = (x, y)  # the input of test_loss_matches_oracle
    for name, bg in (("black_bg", 0.0), ("white_bg", 1.0)):
        t = np.full((H, W, 3), bg, np.float32)
        t[disc] = colour[disc]
        out[name] = (np.full((H, W, 3), bg, np.float32), t)
    yy, xx = np.mgrid[0:H, 0:W]
    texture = 0.02 * np.sin(0.9 * xx + 0.5 * yy)[:, :, None] * np.asarray([1.0, -1.0, 0.5])
    t = np.ones((H, W, 3))
    t[disc] = (colour + texture)[disc]
    t = _f32(t)
    out["late_fit"] = (_f32(_box_blur(t, 3)), t)
    out["equal"] = (t.copy(), t.copy())
    out["const"] = (np.full((H, W, 3), 0.3, np.float32), np.full((H, W, 3), 0.7, np.float32))
    hx, hy = out["noise"][0].copy(), out["noise"][1].copy()
    hx[:, :W // 2] = hy[:, :W // 2] = np.float32(0.6)
    out["half_flat"] = (hx, hy)
    tx, ty = out["black_bg"][0].copy(), out["black_bg"][1]
    tie = rng.random((H, W)) < 0.1
    tx[tie] = ty[tie]
    out["ties"] = (tx, ty)
    assert tuple(out) == PAIR_NAMES
    return {k: (_f32(a), _f32(b)) for k, (a, b) in out.items()}


def weight_maps(H, W):
    """{name: float32 [H, W]}: ``blob`` is zero on half an ellipse that touches the left border (a quarter of the image), one
    elsewhere; ``soft`` has weights in [0.05, 1] outside the same blob."""
    yy, xx = np.mgrid[0:H, 0:W]
    blob = ((yy - 0.5 * H) / (0.4 * H)) ** 2 + (xx / (0.4 * W)) ** 2 <= 1.0
    rng = np.random.default_rng(H * 1000 + W + 7)
    soft = rng.uniform(0.05, 1.0, (H, W)).astype(np.float32)
    soft[blob] = 0.0
    return {"ones": np.ones((H, W), np.float32), "blob": np.where(blob, 0.0, 1.0).astype(np.float32), "soft": soft}


def out_of_reach(weight, radius=5):
    """Pixels whose (2 radius + 1)^2 neighbourhood has weight zero throughout: with radius 5 no weighted window reaches them and
    their own L1 term is switched off, so their gradient is +0.0."""
    m = np.asarray(weight)
    h, w = m.shape
    pad = np.pad(m > 0, radius)
    near = np.zeros((h, w), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            near |= pad[dy:dy + h, dx:dx + w]
    return ~near


def evaluate(pred, target, ssim_weight, weight=None, dtype=np.float64):
    """(loss, l1, ssim, gradient) of the project's restatement at ``dtype``: the truth at float64, the reference arithmetic at
    float32."""
    if weight is None:
        return l1_ssim_loss(pred, target, ssim_weight, dtype=dtype)
    return weighted_l1_ssim_loss(pred, target, weight, ssim_weight, dtype=dtype)


def _reach(H, W, g, wq, x, y, mu, sources, split):
    """sum_q g(p - q) wq_q sum_s mag_s |alpha_s + beta_s (x_p - mu_q) + gamma_s y_p| over the windows q that reach pixel p.
    ``sources``: [(alpha, beta, gamma, magnitude, its own split map or None)]; where ``split`` (or the source's own map) is set the
    beta part is added in magnitude."""
    h, w = mu.shape[:2]
    out = np.zeros((H, W, mu.shape[2]))
    for i in range(len(g)):
        for j in range(len(g)):
            xs, ys = x[i:i + h, j:j + w] - mu, y[i:i + h, j:j + w]
            acc = 0.0
            for al, be, ga, mag, own in sources:
                base, bx = al + ga * ys, be * xs
                sp = split if own is None else (split | own)
                acc = acc + mag * np.where(sp, np.abs(base) + np.abs(bx), np.abs(base + bx))
            out[i:i + h, j:j + w] += g[i] * g[j] * wq * acc
    return out


def scale(pred, target, ssim_weight, weight=None):
    """-> (scale of the gradient [H, W, 3], scale of the SSIM value, scale of the L1 value, the weighted mean of |S|), float64:
    the error of an evaluation with unit roundoff u is (a small count of operations) x u x scale to first order.  ``weight``: the
    map of the weighted loss."""
    x, y = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    H, W, _ = x.shape
    m = np.ones((H, W)) if weight is None else np.asarray(weight, np.float64)
    ws = m.sum()
    wsi = m[5:H - 5, 5:W - 5].sum() if H > 10 and W > 10 else 0.0
    d = x - y
    a = (1.0 - ssim_weight) / (3.0 * ws) if ws > 0 else 0.0
    sc = 3.0 * a * m[:, :, None] * np.abs(np.sign(d))  # the coefficient, the weight, the sum with the SSIM part
    sc_l1 = (m[:, :, None] * np.abs(d)).sum() / (3.0 * ws) if ws > 0 else 0.0
    if not (ssim_weight > 0 and wsi > 0):
        return sc, 0.0, sc_l1, 0.0
    g = gaussian_window()
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ax, ay = np.abs(x), np.abs(y)
    mu, nu = _filt_valid(x, g), _filt_valid(y, g)
    exx, eyy, exy = _filt_valid(x * x, g), _filt_valid(y * y, g), _filt_valid(x * y, g)
    vx_raw, vy_raw = exx - mu * mu, eyy - nu * nu
    A1, A2 = 2 * mu * nu + c1, 2 * (exy - mu * nu) + c2
    B1, B2 = mu * mu + nu * nu + c1, np.maximum(vx_raw, 0) + np.maximum(vy_raw, 0) + c2
    inv = 1.0 / (B1 * B2)
    S = A1 * A2 * inv
    dxx, dxy = -S / B2, 2 * A1 * inv                         # (dExx whatever the clamp decided)
    t1, t2, t3 = 2 * nu * (A2 - A1) * inv, 2 * mu * S / B1, 2 * mu * dxx
    # the magnitudes of the sources
    m_mu, m_nu = _filt_valid(ax, g), _filt_valid(ay, g)
    m_vx, m_vy = exx + mu * mu + _filt_valid(x * x, g), eyy + nu * nu + _filt_valid(y * y, g)
    m_A1 = np.abs(A1) + 2 * np.abs(mu * nu)
    m_A2 = np.abs(A2) + 2 * (np.abs(exy) + np.abs(mu * nu) + _filt_valid(ax * ay, g))
    m_B1 = B1 + mu * mu + nu * nu
    m_B2 = B2 + m_vx + m_vy
    amb_x = np.abs(vx_raw) <= AMBIGUOUS * U * m_vx
    amb_y = np.abs(vy_raw) <= AMBIGUOUS * U * m_vy
    # (alpha, beta, gamma) of dG/ds for the four pointwise sources ...
    dA1 = (-2 * nu * inv - 2 * mu * A2 * inv / B1, -2 * A2 * inv / B2, 2 * inv)
    dA2 = (2 * nu * inv - 2 * mu * A1 * inv / B1, -2 * A1 * inv / B2, 0.0 * inv)
    dB1 = ((-t1 + 2 * t2) / B1, -2 * dxx / B1, -dxy / B1)
    dB2 = (-(t1 - t2) / B2, -4 * dxx / B2, -dxy / B2)
    comb = lambda *parts: tuple(sum(c * p[k] for c, p in parts) for k in range(3))
    zero = 0.0 * inv
    # ... and of the two means: the explicit factors, the chain through A1, A2, B1, and the chain through B2 on its own (it exists
    # only where the variance is not clamped)
    dmu_sure = comb((1.0, (-2 * S / B1 - 2 * dxx, zero, zero)), (2 * nu, dA1), (-2 * nu, dA2), (2 * mu, dB1))
    dnu_sure = comb((1.0, (2 * (A2 - A1) * inv, zero, zero)), (2 * mu, dA1), (-2 * mu, dA2), (2 * nu, dB1))
    dmu_var, dnu_var = comb((-2 * mu, dB2)), comb((-2 * nu, dB2))
    dmu_all, dnu_all = comb((1.0, dmu_sure), (1.0, dmu_var)), comb((1.0, dnu_sure), (1.0, dnu_var))
    never = np.zeros_like(amb_x)
    sources = [dA1 + (m_A1, None), dA2 + (m_A2, None), dB1 + (m_B1, None), dB2 + (m_B2, None),
               # a mean's derivative in one piece where its variance is clearly positive, in two where it is not
               tuple(np.where(amb_x, s, t) for s, t in zip(dmu_sure, dmu_all)) + (m_mu, None),
               tuple(np.where(amb_x, s, zero) for s in dmu_var) + (m_mu, None),
               tuple(np.where(amb_y, s, t) for s, t in zip(dnu_sure, dnu_all)) + (m_nu, None),
               tuple(np.where(amb_y, s, zero) for s in dnu_var) + (m_nu, None),
               # the two decisions of an ambiguous clamp differ by 2 (x_p - mu_q) S / B2, whole
               (zero, np.where(amb_x, 2 * dxx, zero), zero, 1.0 / U, None)]
    mi = m[5:H - 5, 5:W - 5, None]
    adj = lambda q: _filt_full_adjoint(mi * q, g, H, W)
    ss = _reach(H, W, g, mi, x, y, mu, sources, amb_x)
    ss += 2 * adj(np.abs(t1) + np.abs(t2) + np.abs(t3))      # the terms' own last roundings and the filter's
    ss += 2 * ax * 2 * adj(np.abs(dxx)) + ay * 2 * adj(np.abs(dxy))
    sc = sc + ssim_weight / (3.0 * wsi) * ss
    # the SSIM value: the same sources through dS/ds
    s_mu = 2 * nu * A2 * inv - 2 * nu * A1 * inv - 2 * mu * S / B1
    s_nu = 2 * mu * A2 * inv - 2 * mu * A1 * inv - 2 * nu * S / B1
    e_S = np.where(amb_x, np.abs(s_mu) + np.abs(2 * mu * S / B2), np.abs(s_mu + 2 * mu * S / B2)) * m_mu \
        + np.where(amb_y, np.abs(s_nu) + np.abs(2 * nu * S / B2), np.abs(s_nu + 2 * nu * S / B2)) * m_nu \
        + np.abs(A2 * inv) * m_A1 + np.abs(A1 * inv) * m_A2 + np.abs(S) / B1 * m_B1 + np.abs(S) / B2 * m_B2 + 2 * np.abs(S)
    sc_ssim = float((mi * e_S).sum() / (3.0 * wsi))
    return sc, sc_ssim, sc_l1, float((mi * np.abs(S)).sum() / (3.0 * wsi))


def ratio(got, truth, sc):
    """|got - truth| / (U scale) element by element; 0 where both the error and the scale are zero, inf where only the scale is."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(truth, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err > 0, err / (U * np.asarray(sc, np.float64)), 0.0)


QS = (0.5, 0.99, 0.999, 1.0)
Q_NAMES = ("median", "p99", "p99.9", "max")


def quantiles(r):
    return tuple(float(np.quantile(r, q)) for q in QS)


def value_bounds(ssim_weight, sc_ssim, sc_l1, abs_s_mean, loss, n_terms, f_ssim):
    """(bound of loss, of l1, of ssim) for an evaluation that sums its terms in fp32 along chains of at most ``n_terms`` additions
    and computes S within ``f_ssim`` x U x sc_ssim: the chain bound n U sum|term| / n_total on both means, and the three
    operations of  (1 - w) l1 + w (1 - ssim)."""
    b_l1 = (n_terms + 2) * U * sc_l1               # |x - y| is exact to one rounding; the sum; the normaliser
    b_ssim = f_ssim * U * sc_ssim + (n_terms + 2) * U * abs_s_mean
    b_loss = (1.0 - ssim_weight) * b_l1 + ssim_weight * b_ssim + 4 * U * (abs(loss) + ssim_weight)
    return b_loss, b_l1, b_ssim


_REF = {}
_INPUTS = {}


def inputs(H, W):
    """(pairs, weight maps) of a size, built once; nobody writes to them."""
    if (H, W) not in _INPUTS:
        _INPUTS[(H, W)] = (pairs(H, W), weight_maps(H, W))
        for a in [i for pr in _INPUTS[(H, W)][0].values() for i in pr] + list(_INPUTS[(H, W)][1].values()):
            a.setflags(write=False)
    return _INPUTS[(H, W)]


def reference_of(x, y, ssim_weight, m=None):
    """Everything a comparison needs for one input: the float64 truth, the float32 restatement, the scales, the restatement's
    ratios and their quantiles."""
    lo, l1, ssim, g64 = evaluate(x, y, ssim_weight, m)
    lo32, l132, ssim32, g32 = evaluate(x, y, ssim_weight, m, np.float32)
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    sc, sc_ssim, sc_l1, s_abs = scale(x, y, ssim_weight, m)
    r32 = ratio(g32, g64, sc)
    return dict(values=(lo, l1, ssim), grad=g64, values32=(lo32, l132, ssim32), grad32=g32, scale=sc, scale_ssim=sc_ssim,
                scale_l1=sc_l1, s_abs=s_abs, ratio32=r32, q32=quantiles(r32),
                ratio32_ssim=abs(ssim32 - ssim) / (U * sc_ssim) if sc_ssim > 0 else 0.0)


def reference(H, W, name, ssim_weight, map_name=None):
    """``reference_of`` for a named pair (and weight map) of a size, computed once and shared.  The weight of the SSIM term is an
    fp32 input like the images (the C ABI takes a float): the truth is taken at its fp32 value."""
    ssim_weight = float(np.float32(ssim_weight))
    key = (H, W, name, ssim_weight, map_name)
    if key not in _REF:
        P, M = inputs(H, W)
        _REF[key] = reference_of(*P[name], ssim_weight, None if map_name is None else M[map_name])
    return _REF[key]


# The cases F_REF is taken over: every pair under every weight map (None: the unweighted statement) at 64 x 80, ssim_weight 0.2; the
# unweighted pairs again at 1.0, where no L1 term hides anything; one 120 x 176 pair under every map.
HOST_CASES = [(64, 80, n, 0.2, mp) for n in PAIR_NAMES for mp in (None,) + WEIGHT_NAMES] + \
    [(64, 80, n, 1.0, None) for n in PAIR_NAMES] + [(120, 176, "late_fit", 0.2, mp) for mp in (None,) + WEIGHT_NAMES]


def case_label(H, W, name, sw, mp):
    return f"{H}x{W} w={sw} {name}" + (f" / {mp}" if mp else "")


def table_row(label, q, q_ssim=None):
    row = f"{label:34s} " + " ".join(f"{v:9.4f}" for v in q)
    return row + (f"   {q_ssim:9.4f}" if q_ssim is not None else "")


def host_report():
    """The numpy-float32 table of profiles/loss_calibration.txt and the measured (F_ref, F_ref of the SSIM value)."""
    lines = [f"{'case (numpy float32 restatement)':34s} " + " ".join(f"{n:>9s}" for n in Q_NAMES) + "   ssim value"]
    f_ref = f_ssim = 0.0
    for c in HOST_CASES:
        r = reference(*c)
        lines.append(table_row(case_label(*c), r["q32"], r["ratio32_ssim"]))
        f_ref, f_ssim = max(f_ref, r["q32"][3]), max(f_ssim, r["ratio32_ssim"])
    q_s = quantiles(np.asarray([reference(*c)["ratio32_ssim"] for c in HOST_CASES]))
    lines.append(table_row("ssim value over the cases", q_s))
    lines.append(f"measured F_ref = {f_ref:.4f} (recorded F_REF = {F_REF}); measured F_ref,ssim = {f_ssim:.4f} "
                 f"(recorded F_REF_SSIM = {F_REF_SSIM})")
    return "\n".join(lines), f_ref, f_ssim


if __name__ == "__main__":
    print(host_report()[0])
