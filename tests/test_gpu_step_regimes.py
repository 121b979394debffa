"""GPU: the kernels of the training step around the frame path (densification, the pair sort, Adam, the image loss)
beyond the input sizes at which each of them takes another code path -- a second trip of a one-workgroup scan, a capped
grid with a stride loop, the streaming instantiation -- and at the argument combinations the other parity tests leave
out.  Every size below is the smallest that crosses its threshold, plus a ragged one past it; the thresholds are
constants of the kernels and are restated here beside the source line they come from: whoever moves one moves the test.

All entry points are called through the C ABI (gaussian._lib); the references are oracle/densify_ref.py,
oracle/train_ref.py and numpy's stable argsort.  Lines that start with REGIME carry the worst error / tolerance of each
comparison (profiles/step_kernel_regimes.txt records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import densify_ref, train_ref
from test_gpu_densify import check_matches_oracle, random_set

pytestmark = pytest.mark.gpu

# densify.hip: densify_classify_kernel is launched with 256 threads per workgroup (`blockIdx.x * 256 + threadIdx.x`) ...
DENSIFY_BLOCK = 256
# ... and densify_scan_kernel, one workgroup of 1024 threads, scans 1024 block counts per trip (`base += 1024`)
DENSIFY_SCAN_TRIP = 1024
DENSIFY_ONE_TRIP = DENSIFY_BLOCK * DENSIFY_SCAN_TRIP  # 262,144 Gaussians: the most that one trip covers

# radix_sort.hip: RS_TILE = RS_THREADS * RS_KPT = 2048 pairs per workgroup; row_scan_kernel scans RS_THREADS = 256
# workgroup histograms per trip (`b0 += RS_THREADS`)
RS_TILE = 2048
RS_SCAN_TRIP = 256
SORT_ONE_TRIP = RS_TILE * RS_SCAN_TRIP  # 524,288 pairs

# adam.hip, adam_step_impl: `if (blocks > 256 * 16) blocks = 256 * 16`, 256 threads of one float4 each
ADAM_GRID_CAP = 256 * 16 * 256 * 4  # 4,194,304 elements in one launch without the stride loop
# adam.hip, gs_adam_step_multi: `if (blocks > 256 * 8) blocks = 256 * 8`, per range
ADAM_MULTI_GRID_CAP = 256 * 8 * 256 * 4  # 2,097,152 elements per range
# adam.hip: GS_ADAM_NT_BYTES = 300 MiB of the four arrays (16 bytes per element) -> the NT = true instantiation;
# gs_adam_step* compare it with the RANGE's length, gs_adam_step_multi with n
ADAM_NT_ELEMS = (300 << 20) // 16  # 19,660,800 elements

# loss.hip: loss_finish_kernel is one workgroup of 256 threads (`i += 256` over the partial sums)
LOSS_FINISH_TRIP = 256
# loss.hip: GS_LOSS_SH = 52 gradient rows and FCW = GS_LOSS_FT - 2 * 15 = 482 flat columns per workgroup
LOSS_SH, LOSS_FCW = 52, 482
# loss.hip: l1_only_kernel runs min(ceil(n / (256 * 4)), L1_BLOCKS = 1024) workgroups of 256 threads
L1_BLOCKS, L1_PER_BLOCK = 1024, 256 * 4

BETAS_EPS = (0.9, 0.99, 1e-8)
NAN_BITS = 0x7FC0BEEF  # a quiet NaN that no computation here produces


def report(what, **ratios):
    print("REGIME", what + ":", ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def bits(t):
    return t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- 1. densification
def oracle_classes(arrays, grad, act, agg, use_clone, use_split):
    """Class of every INPUT Gaussian (0 deleted, 1 kept, 2 kept + cloned, 3 kept + split) by the rules of
    oracle/densify_ref.py; the caller ties it to the oracle's own counts."""
    f = np.float32
    _, _, scale, opa, _ = arrays
    a = np.abs(scale) if act == "abs" else np.exp(scale)
    norm = np.sqrt((a * a).sum(-1, dtype=f))
    keep = (opa > f(densify_ref.inverse_sigmoid(0.02))) & (norm < f(0.17))
    g = np.abs(grad).max(-1) if agg == "max" else np.abs(grad).mean(-1, dtype=f)
    dens = keep & (g > f(0.0002))
    cls = keep.astype(np.int32)
    cls[dens & (norm <= f(0.05)) & use_clone] = 2
    cls[dens & (norm > f(0.05)) & use_split] = 3
    return cls


@pytest.mark.parametrize("n,act,kw", [
    (DENSIFY_ONE_TRIP, "abs", {}),          # exactly 1024 blocks: one full trip
    (DENSIFY_ONE_TRIP + 1, "abs", {}),      # 1025 blocks: the second trip scans one block
    (600_001, "abs", {}),                   # three trips, the last one ragged
    (DENSIFY_ONE_TRIP + 1, "abs", {"grad_aggregation": "mean"}),
    (DENSIFY_ONE_TRIP + 1, "abs", {"use_clone": False}),
    (DENSIFY_ONE_TRIP + 1, "abs", {"use_split": False}),
    (DENSIFY_ONE_TRIP + 1, "exp", {}),
], ids=["1024blk", "1025blk", "600001", "mean", "no_clone", "no_split", "exp"])
def test_densify_beyond_one_scan_trip(gpu, n, act, kw):
    """gs_densify_classify + gs_densify_apply against the oracle where densify_scan_kernel carries its running totals
    from one trip of 1024 block counts into the next.  Bit-equal outputs pin the output order, hence every block
    offset."""
    arrays, grad, draws = random_set(n, 3, act)
    kw = dict(dict(scale_activation=act, grad_aggregation="max", use_clone=True, use_split=True), **kw)
    counts, ratios = check_matches_oracle(gpu, arrays, grad, draws, **kw)
    # a dropped carry of one counter can only show if that counter is non-zero in every trip's share of the input
    cls = oracle_classes(arrays, grad, act, kw["grad_aggregation"], kw["use_clone"], kw["use_split"])
    assert ((cls > 0).sum(), (cls == 2).sum(), (cls == 3).sum()) == counts
    for lo in range(0, n, DENSIFY_ONE_TRIP):
        c = cls[lo:lo + DENSIFY_ONE_TRIP]
        if len(c) < DENSIFY_BLOCK:  # the one Gaussian in the second trip of n = 262,145 has one class; the totals,
            continue                # which leave the kernel through the same carry, cover that trip
        assert (c > 0).any() and ((c == 2).any() or not kw["use_clone"]) and ((c == 3).any() or not kw["use_split"])
    if kw["grad_aggregation"] == "mean":  # a max / mean mix-up changes the counts
        assert densify_ref.adaptive_control(*arrays, grad, 0.05, 0.17, *draws, **dict(kw, grad_aggregation="max"))[5] \
            != counts
    report(f"densify n={n} {act} {kw['grad_aggregation']} clone={kw['use_clone']} split={kw['use_split']} "
           f"counts={counts}", **ratios)


@pytest.mark.parametrize("short", ["none", "capacity", "n_eps"])
def test_densify_apply_leaves_short_outputs_alone(gpu, short):
    """densify_apply_kernel returns before its first store when the counts exceed `capacity` or the split count exceeds
    `n_eps`: return code 0 and not one byte of the outputs written.  ("none": the same call with room for everything
    overwrites every element of the pattern, so the two other cases are not vacuous.)"""
    from gaussian import _lib

    n = 5_000
    arrays, grad, draws = random_set(n, 3, "abs")
    opts = _lib.GsDensifyOpts(0.05, 0.17, 0.0002, 0.01, 0, 0, 1, 1, 3)
    t = [dev(a, gpu) for a in arrays]
    g = dev(grad, gpu)
    ws = torch.empty(int(_lib.gs_densify_workspace_bytes(n)), dtype=torch.uint8, device=gpu)
    counts = torch.zeros(4, dtype=torch.int64, device=gpu)
    _lib.check(_lib.gs_densify_classify(t[2].data_ptr(), t[3].data_ptr(), g.data_ptr(), n, C.byref(opts),
                                        counts.data_ptr(), ws.data_ptr(), ws.numel(), stream()), "gs_densify_classify")
    kept, cloned, split, total = (int(v) for v in counts.cpu())
    assert total == kept + cloned + split and cloned > 1 and split > 1
    # the tensors are as large as a complete result, whatever size the call is told: nothing here can leave them
    e1, e2 = (dev(d[:split], gpu) for d in draws)
    out = [torch.full((total,) + a.shape[1:], NAN_BITS, dtype=torch.int32, device=gpu) for a in arrays]
    capacity = total - 1 if short == "capacity" else total
    n_eps = split - 1 if short == "n_eps" else split
    rc = _lib.gs_densify_apply(*(x.data_ptr() for x in t), g.data_ptr(), n, C.byref(opts), e1.data_ptr(), e2.data_ptr(),
                               n_eps, *(o.data_ptr() for o in out), capacity, counts.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream())
    assert rc == 0
    for o in out:
        if short == "none":
            assert not bool((o == NAN_BITS).any())
        else:
            assert bool((o == NAN_BITS).all())


# ---------------------------------------------------------------------------------------------------- 2. the pair sort
GUARD_K = (0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C)  # what the two key buffers hold where no pair is
GUARD_V = (0x1EADBEE0, 0x2EADBEE1)
SORT_SLACK = 64  # elements behind `capacity` in every buffer (guards; the kernels are never told about them)


def sort_pairs(gpu, keys, count, cap, begin_bit, end_bit, stale_hist=None):
    """gs_sort_pairs_bits on keys[:min(len, cap)] (values = positions) with the device count `count`.  Both buffer pairs
    are cap + SORT_SLACK long and hold GUARD_K / GUARD_V wherever no input pair is.
    -> (keys, values) of the buffer the call names and of the other one, as numpy arrays, and the flag."""
    from gaussian import _lib

    m = min(len(keys), cap)
    k = [torch.full((cap + SORT_SLACK,), g, dtype=torch.int64, device=gpu) for g in GUARD_K]
    v = [torch.full((cap + SORT_SLACK,), g, dtype=torch.int32, device=gpu) for g in GUARD_V]
    k[0][:m] = dev(keys[:m].view(np.int64), gpu)
    v[0][:m] = torch.arange(m, dtype=torch.int32, device=gpu)
    cnt = torch.tensor([count, 0], dtype=torch.int32, device=gpu)
    tmp = torch.zeros(_lib.gs_sort_pairs_tmp_bytes(cap), dtype=torch.uint8, device=gpu)
    if stale_hist is not None:  # what an earlier, larger sort could have left in the histogram rows
        tmp.view(torch.int32).fill_(stale_hist)
    in1 = C.c_int(-1)
    _lib.check(_lib.gs_sort_pairs_bits(k[0].data_ptr(), v[0].data_ptr(), k[1].data_ptr(), v[1].data_ptr(),
                                       cnt.data_ptr(), cap, begin_bit, end_bit, tmp.data_ptr(), tmp.numel(),
                                       C.byref(in1), stream()), "gs_sort_pairs_bits")
    assert in1.value in (0, 1)
    res = [(k[b].cpu().numpy().view(np.uint64), v[b].cpu().numpy().view(np.uint32)) for b in (in1.value, 1 - in1.value)]
    return res[0], res[1], in1.value


def check_sorted(gpu, keys, n, cap, begin_bit, end_bit, count=None, **kw):
    """The first n pairs are the stable sort of the input by key bits [begin_bit, end_bit); whatever lies behind them
    in either buffer pair, up to the end of the allocation, is what was there before the call."""
    (ks, vs), (ko, vo), in1 = sort_pairs(gpu, keys, n if count is None else count, cap, begin_bit, end_bit, **kw)
    npass = (end_bit - begin_bit + 7) // 8
    assert in1 == (npass & 1)
    sel = (keys[:n] >> np.uint64(begin_bit)) & np.uint64((1 << (end_bit - begin_bit)) - 1)
    order = np.argsort(sel, kind="stable")
    assert np.array_equal(ks[:n], keys[:n][order])
    assert np.array_equal(vs[:n], order.astype(np.uint32))  # stability
    m = min(len(keys), cap)
    before_k = [np.full(cap + SORT_SLACK, g, np.uint64) for g in GUARD_K]
    before_v = [np.full(cap + SORT_SLACK, g, np.uint32) for g in GUARD_V]
    before_k[0][:m], before_v[0][:m] = keys[:m], np.arange(m, dtype=np.uint32)
    assert np.array_equal(ks[n:], before_k[in1][n:]) and np.array_equal(vs[n:], before_v[in1][n:])
    assert np.array_equal(ko[n:], before_k[1 - in1][n:]) and np.array_equal(vo[n:], before_v[1 - in1][n:])


def tile_depth_keys(rng, n):
    """test_gpu_kernels.test_sort_pairs' keys: tile ids below 700 over 40 distinct depths -- many ties"""
    tiles = rng.integers(0, 700, n).astype(np.uint64)
    depth = rng.integers(0, 40, n).astype(np.uint64) * np.uint64(0x01000193) % np.uint64(1 << 32)
    return (tiles << np.uint64(32)) | depth


@pytest.mark.parametrize("n", [SORT_ONE_TRIP, SORT_ONE_TRIP + 1, 1_200_003])
def test_sort_pairs_beyond_one_scan_trip(gpu, n):
    """256 workgroups exactly, 257, and three ragged trips of row_scan_kernel's carry loop."""
    rng = np.random.default_rng(n + 11)
    check_sorted(gpu, tile_depth_keys(rng, n + 1000), n, n + 1000, 0, 32 + 10)


@pytest.mark.parametrize("n", [5_000, SORT_ONE_TRIP + 1])
def test_sort_pairs_full_width_keys(gpu, n):
    """All 64 key bits, eight passes; keys drawn (with repeats) from a pool of random 64-bit values."""
    rng = np.random.default_rng(n + 12)
    pool = rng.integers(0, 1 << 64, max(n // 4, 1), dtype=np.uint64)
    keys = pool[rng.integers(0, len(pool), n)]
    assert (keys >> np.uint64(63)).any() and not (keys >> np.uint64(63)).all()
    check_sorted(gpu, keys, n, n + 1000, 0, 64)


@pytest.mark.parametrize("n", [5_000, SORT_ONE_TRIP + 1])
def test_sort_pairs_middle_bits(gpu, n):
    """begin_bit = 32, end_bit = 48: the random bits below 32 must not influence the order (no key bit at or above
    end_bit is set: what a partial last digit does with those is not specified)."""
    rng = np.random.default_rng(n + 13)
    keys = (rng.integers(0, 1 << 16, n).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, n).astype(np.uint64)
    check_sorted(gpu, keys, n, n + 1000, 32, 48)


@pytest.mark.parametrize("end_bit,npass", [(40, 5), (48, 6), (33, 5)])
def test_sort_pairs_pass_parity(gpu, end_bit, npass):
    """An odd and an even number of passes: `sorted_in_buffer1` names the buffer that holds the result (check_sorted
    reads the result from the buffer it names and finds the other one's tail untouched)."""
    assert (end_bit + 7) // 8 == npass
    n = 5_000
    keys = np.random.default_rng(end_bit).integers(0, 1 << end_bit, n).astype(np.uint64)
    keys[::3] = keys[1]  # ties
    check_sorted(gpu, keys, n, n + 1000, 0, end_bit)


def test_sort_pairs_count_above_capacity(gpu):
    """A device count of capacity + 5 sorts exactly `capacity` pairs and touches nothing behind them."""
    cap = 5_000
    keys = tile_depth_keys(np.random.default_rng(14), cap)
    check_sorted(gpu, keys, cap, cap, 0, 42, count=cap + 5)


@pytest.mark.parametrize("end_bit", [42, 40])
def test_sort_pairs_capacity_far_above_count(gpu, end_bit):
    """capacity 1,000,000 (489 workgroups, 488 of them idle), 5 pairs, the histogram rows holding an earlier sort's
    values: positions [5, capacity) of both buffer pairs still hold what was there before the call."""
    keys = tile_depth_keys(np.random.default_rng(15), 5) & np.uint64((1 << end_bit) - 1)
    check_sorted(gpu, keys, 5, 1_000_000, 0, end_bit, stale_hist=7)


# ---------------------------------------------------------------------------------------------------- 3. Adam
def tables(ends, lrs):
    return (C.c_int64 * len(ends))(*ends), (C.c_float * len(lrs))(*lrs)


def i64s(*v):
    return (C.c_int64 * len(v))(*v)


class AdamState:
    """p, m, v on the device (+ the statistic) and the entry points over them; all steps share `ends` / `lrs`."""

    def __init__(self, gpu, p0, ends, lrs, stat=None, stat_range=(0, 0), stat_mode=0):
        from gaussian import _lib

        self.lib, self.n = _lib, len(p0)
        self.p = dev(p0, gpu)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.ends_l, self.lrs_l = list(ends), list(lrs)
        self.ends, self.lr = tables(ends, lrs)
        self.stat, self.stat_range, self.stat_mode = stat, stat_range, stat_mode

    def _head(self, g):
        return (self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n)

    def _tail(self, step):
        return (len(self.ends_l), self.ends, self.lr, *BETAS_EPS, step,
                self.stat.data_ptr() if self.stat is not None else None, *self.stat_range, self.stat_mode)

    def one(self, g, step):
        self.lib.check(self.lib.gs_adam_step(*self._head(g), *self._tail(step), stream()), "gs_adam_step")

    def ranges(self, g, step, cuts):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            self.lib.check(self.lib.gs_adam_step_range(*self._head(g), lo, hi, *self._tail(step), stream()),
                           "gs_adam_step_range")

    def multi(self, g, step, los, his, skip=None, grad_scale=1.0):
        self.lib.check(self.lib.gs_adam_step_multi(*self._head(g), len(los), i64s(*los), i64s(*his), i64s(*los),
                                                   *self._tail(step), skip, grad_scale, stream()), "gs_adam_step_multi")

    def equal(self, other):
        return same_bits(self.p, other.p) and same_bits(self.m, other.m) and same_bits(self.v, other.v)


def oracle_adam(p0, grads, ends, lrs, lo=0, hi=None):
    """oracle/train_ref.adam_step group by group over elements [lo, hi), one step per gradient -> (p, m, v)"""
    hi = len(p0) if hi is None else hi
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step, g in enumerate(grads, 1):
        a = 0
        for b, lr in zip(ends, lrs):
            s = slice(max(a, lo), min(b, hi))
            if s.start < s.stop:
                p[s], m[s], v[s] = train_ref.adam_step(p[s], g[s], m[s], v[s], lr, *BETAS_EPS, step)
            a = b
    return p, m, v


def adam_ratio(p_gpu, want):
    """worst |p - oracle| / (1e-6 max(1, |p|max)): the tolerance of test_gpu_train.test_adam_matches_oracle_and_torch"""
    return float(np.abs(p_gpu.cpu().numpy() - want).max() / (1e-6 * max(1.0, float(np.abs(want).max()))))


def normal32(rng, n):
    return rng.standard_normal(n, dtype=np.float32)


def test_adam_grid_stride(gpu):
    """gs_adam_step over more elements than its capped grid covers in one trip, with the statistic on a ragged range
    that reaches into the second trip: bit-equal to the same data through gs_adam_step_range in pieces below the cap,
    and within the tolerance of the oracle."""
    n = ADAM_GRID_CAP + 4_099
    rng = np.random.default_rng(31)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(2)]
    ends, lrs = [1_000_003, 3_000_000, n], [0.03, 0.004, 0.02]
    srange = (1_000_001, ADAM_GRID_CAP + 2_000)
    run = []
    for kind in ("one", "pieces"):
        stat = torch.zeros(srange[1] - srange[0], device=gpu)
        a = AdamState(gpu, p0, ends, lrs, stat, srange, 1)
        for step, g in enumerate(grads, 1):
            g = dev(g, gpu)
            if kind == "one":
                a.one(g, step)
            else:
                cuts = [0, 1_500_001, 3_000_002, n]
                assert max(np.diff(cuts)) <= ADAM_GRID_CAP
                a.ranges(g, step, cuts)
        run.append(a)
    assert run[0].equal(run[1]) and same_bits(run[0].stat, run[1].stat)
    want = np.maximum(np.abs(grads[0]), np.abs(grads[1]))[srange[0]:srange[1]]
    assert np.array_equal(run[0].stat.cpu().numpy(), want)
    ratio = adam_ratio(run[0].p, oracle_adam(p0, grads, ends, lrs)[0])
    report(f"adam grid stride n={n}", p=ratio)
    assert ratio <= 1.0


def test_adam_multi_grid_stride(gpu):
    """gs_adam_step_multi with one range beyond its per-range grid cap and a second short one: bit-equal to
    gs_adam_step_range over the same elements in pieces, elements outside the ranges untouched."""
    n = ADAM_GRID_CAP + 4_099
    rng = np.random.default_rng(32)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(2)]
    ends, lrs = [1_000_003, 3_000_000, n], [0.03, 0.004, 0.02]
    long_hi = ADAM_MULTI_GRID_CAP + 4_101
    los, his = [0, long_hi + 3], [long_hi, long_hi + 3 + 1_003]
    assert los[1] % 4 == 0 and his[0] - los[0] > ADAM_MULTI_GRID_CAP
    a, b = AdamState(gpu, p0, ends, lrs), AdamState(gpu, p0, ends, lrs)
    for step, g in enumerate(grads, 1):
        g = dev(g, gpu)
        a.multi(g, step, los, his)
        b.ranges(g, step, [0, 1_000_001, long_hi])
        b.ranges(g, step, [los[1], his[1]])
    assert a.equal(b)
    p = a.p.cpu().numpy()
    assert np.array_equal(p[long_hi:los[1]], p0[long_hi:los[1]]) and np.array_equal(p[his[1]:], p0[his[1]:])
    assert not bool(a.m[long_hi:los[1]].any()) and not bool(a.m[his[1]:].any()) and not bool(a.v[his[1]:].any())
    want = oracle_adam(p0, grads, ends, lrs, 0, long_hi)[0]
    want[los[1]:his[1]] = oracle_adam(p0, grads, ends, lrs, los[1], his[1])[0][los[1]:his[1]]
    ratio = adam_ratio(a.p, want)
    report(f"adam multi grid stride, ranges {list(zip(los, his))}", p=ratio)
    assert ratio <= 1.0


@pytest.fixture(scope="module")
def streaming_case(gpu):
    """19.7 M elements, two steps: the inputs, the oracle's result, and the result of the plain (NT = false)
    instantiation, which two gs_adam_step_range halves below GS_ADAM_NT_BYTES take.  Shared, read-only."""
    n = 19_700_003
    assert n > ADAM_NT_ELEMS
    rng = np.random.default_rng(33)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(2)]
    ends, lrs = [6_000_001, 13_000_000, n], [0.03, 0.004, 0.02]  # one boundary inside a float4
    half = 9_850_000  # a multiple of 4, so that gs_adam_step_multi can cut there too
    assert half <= ADAM_NT_ELEMS and n - half <= ADAM_NT_ELEMS and half % 4 == 0
    g_dev = [dev(g, gpu) for g in grads]
    plain = AdamState(gpu, p0, ends, lrs)
    for step, g in enumerate(g_dev, 1):
        plain.ranges(g, step, [0, half + 1, n])  # (the cut itself ragged)
    want = oracle_adam(p0, grads, ends, lrs)[0]
    return dict(n=n, p0=p0, g_dev=g_dev, ends=ends, lrs=lrs, half=half, plain=plain, want=want)


@pytest.mark.parametrize("entry", ["one", "multi"])
def test_adam_streaming_instantiation(gpu, streaming_case, entry):
    """The NT = true kernels (non-temporal loads / stores of gradient and moments), which nothing else compares with
    anything: one gs_adam_step launch beyond GS_ADAM_NT_BYTES, and gs_adam_step_multi, whose switch looks at n."""
    c = streaming_case
    a = AdamState(gpu, c["p0"], c["ends"], c["lrs"])
    for step, g in enumerate(c["g_dev"], 1):
        if entry == "one":
            a.one(g, step)
        else:
            a.multi(g, step, [0, c["half"]], [c["half"], c["n"]])
    assert a.equal(c["plain"])
    ratio = adam_ratio(a.p, c["want"])
    report(f"adam streaming {entry} n={c['n']}", p=ratio)
    assert ratio <= 1.0


SHARD = dict(n=4_003, lo=1_001, hi=2_999, base=1_000, stat=(900, 2_503))  # the statistic begins before the shard
MOMENT_GUARD = 8  # floats in front of the shard's moments (keeps them 16-byte aligned)


def sharded_run(gpu, skip_value=None, steps=2):
    """gs_adam_step_sharded on SHARD with the moments of [base, hi) only, inside an allocation of guard values that is
    long enough for ANY index below n (a mis-based kernel lands in the guards, not outside the tensor).
    -> (p, m allocation, v allocation, stat allocation) and the inputs"""
    from gaussian import _lib

    s = SHARD
    rng = np.random.default_rng(34)
    p0, grads = normal32(rng, s["n"]), [normal32(rng, s["n"]) for _ in range(steps)]
    ends, lrs = [7, 1_310, 2_311, s["n"]], [0.03, 0.02, 0.003, 0.004]
    et, lt = tables(ends, lrs)
    p = dev(p0, gpu)
    m = torch.full((MOMENT_GUARD + s["n"] + MOMENT_GUARD,), 123.0, device=gpu)
    v = torch.full_like(m, 321.0)
    live = slice(MOMENT_GUARD + s["lo"] - s["base"], MOMENT_GUARD + s["hi"] - s["base"])
    m[live], v[live] = 0.0, 0.0
    stat = torch.full((3 + s["stat"][1] - s["stat"][0] + 3,), 0.5, device=gpu)
    flag = None if skip_value is None else torch.tensor([skip_value], dtype=torch.int64, device=gpu)
    for step, g in enumerate(grads, 1):
        g = dev(g, gpu)
        _lib.check(_lib.gs_adam_step_sharded(p.data_ptr(), g.data_ptr(), m.data_ptr() + 4 * MOMENT_GUARD,
                                             v.data_ptr() + 4 * MOMENT_GUARD, s["n"], s["lo"], s["hi"], s["base"],
                                             len(ends), et, lt, *BETAS_EPS, step, stat.data_ptr() + 4 * 3, *s["stat"], 2,
                                             None if flag is None else flag.data_ptr(), stream()),
                   "gs_adam_step_sharded")
    return (p, m, v, stat), (p0, grads, ends, lrs, live)


def test_adam_sharded_moments_with_a_ragged_range(gpu):
    """moment_base != 0 and a range that begins and ends inside a float4: the shard's parameters and moments are, bit
    for bit, what gs_adam_step gives those elements on full arrays; everything else -- parameters outside the range,
    the guards around the shard's moments, the unused moment slot of element `moment_base`, the statistic's guards --
    is untouched."""
    s = SHARD
    (p, m, v, stat), (p0, grads, ends, lrs, live) = sharded_run(gpu)
    full = AdamState(gpu, p0, ends, lrs)
    for step, g in enumerate(grads, 1):
        full.one(dev(g, gpu), step)
    lo, hi = s["lo"], s["hi"]
    assert same_bits(p[lo:hi], full.p[lo:hi]) and same_bits(m[live], full.m[lo:hi]) and same_bits(v[live], full.v[lo:hi])
    pc = p.cpu().numpy()
    assert np.array_equal(pc[:lo], p0[:lo]) and np.array_equal(pc[hi:], p0[hi:])
    for t, guard in ((m, 123.0), (v, 321.0)):
        assert bool((t[:live.start] == guard).all()) and bool((t[live.stop:] == guard).all())
    assert live.start == MOMENT_GUARD + 1  # the slot of element moment_base itself is one of those
    assert bool((stat[:3] == 0.5).all()) and bool((stat[-3:] == 0.5).all())
    # the statistic saw the elements of [lo, hi) only: its first lo - stat_begin entries are unchanged
    want = np.full(s["stat"][1] - s["stat"][0], 0.5, np.float32)
    for g in grads:
        want[lo - s["stat"][0]:] += np.abs(g[lo:s["stat"][1]])
    assert np.allclose(stat[3:-3].cpu().numpy(), want, rtol=1e-6, atol=0)
    ratio = adam_ratio(p[lo:hi], oracle_adam(p0, grads, ends, lrs, lo, hi)[0][lo:hi])
    report("adam sharded [1001, 2999) moment_base 1000", p=ratio)
    assert ratio <= 1.0


def test_adam_skip_flag_sharded(gpu):
    """skip_if_nonzero on the plain kernel: a counter of 1 leaves p, m, v and the statistic bit-unchanged, a counter of
    0 is the call without a flag."""
    ran, (p0, _, _, _, live) = sharded_run(gpu)
    zero, _ = sharded_run(gpu, skip_value=0)
    assert all(same_bits(a, b) for a, b in zip(ran, zero))
    assert not np.array_equal(ran[0].cpu().numpy(), p0)
    p, m, v, stat = sharded_run(gpu, skip_value=1)[0]
    assert np.array_equal(p.cpu().numpy(), p0)
    assert not bool(m[live].any()) and not bool(v[live].any()) and bool((stat == 0.5).all())
    assert bool((m[:live.start] == 123.0).all()) and bool((m[live.stop:] == 123.0).all())


def test_adam_skip_flag_multi(gpu):
    n = 4_003
    rng = np.random.default_rng(35)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(2)]
    ends, lrs = [7, 1_310, 2_311, n], [0.03, 0.02, 0.003, 0.004]
    los, his = [0, 1_200], [1_199, n]
    res = {}
    for value in (None, 0, 1):
        a = AdamState(gpu, p0, ends, lrs, torch.full((1_000,), 0.5, device=gpu), (1_100, 2_100), 1)
        flag = None if value is None else torch.tensor([value], dtype=torch.int64, device=gpu)
        for step, g in enumerate(grads, 1):
            a.multi(dev(g, gpu), step, los, his, skip=None if flag is None else flag.data_ptr())
        res[value] = a
    assert res[None].equal(res[0]) and same_bits(res[None].stat, res[0].stat)
    assert not np.array_equal(res[None].p.cpu().numpy(), p0)
    a = res[1]
    assert np.array_equal(a.p.cpu().numpy(), p0) and not bool(a.m.any()) and not bool(a.v.any())
    assert bool((a.stat == 0.5).all())


def test_adam_grad_scale(gpu):
    """gs_adam_step_multi's grad_scale: 1/3 against the oracle fed g * float32(1/3) computed in fp32; 1 bit-equal to
    gs_adam_step."""
    n = 10_007
    rng = np.random.default_rng(36)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(2)]
    ends, lrs = [7, 1_310, 2_311, n], [0.03, 0.02, 0.003, 0.004]
    los, his = [0, 4_000], [4_000, n]
    third = np.float32(1.0 / 3.0)
    one, unit, scaled = (AdamState(gpu, p0, ends, lrs) for _ in range(3))
    for step, g in enumerate(grads, 1):
        g = dev(g, gpu)
        one.one(g, step)
        unit.multi(g, step, los, his, grad_scale=1.0)
        scaled.multi(g, step, los, his, grad_scale=float(third))
    assert unit.equal(one)
    assert not same_bits(scaled.p, one.p)
    ratio = adam_ratio(scaled.p, oracle_adam(p0, [g * third for g in grads], ends, lrs)[0])
    report("adam grad_scale 1/3", p=ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("entry", ["one", "ranges", "multi"])
def test_adam_statistic_range_inside_float4s(gpu, entry, mode):
    """A statistic range whose two ends fall inside float4s of the vector body (and, for the cut launches, next to the
    cuts): max exact, sum to rtol 1e-6, the guard elements on either side of the statistic unchanged."""
    n, sb, se = 1_003, 5, 310
    rng = np.random.default_rng(37)
    p0, grads = normal32(rng, n), [normal32(rng, n) for _ in range(3)]
    init = np.abs(normal32(rng, se - sb)) * 0.5
    buf = torch.full((3 + se - sb + 3,), -7.0, device=gpu)
    buf[3:-3] = dev(init, gpu)
    a = AdamState(gpu, p0, [7, 310, 311, 640, n], [0.03, 0.02, 0.003, 0.004, 0.005], buf[3:], (sb, se), mode)
    want = init.copy()
    for step, g in enumerate(grads, 1):
        gd = dev(g, gpu)
        if entry == "one":
            a.one(gd, step)
        elif entry == "ranges":
            a.ranges(gd, step, [0, 7, 309, n])
        else:
            a.multi(gd, step, [0, 308, 312], [308, 312, n])
        want = np.maximum(want, np.abs(g[sb:se])) if mode == 1 else want + np.abs(g[sb:se])
    got = buf.cpu().numpy()
    assert np.all(got[:3] == -7.0) and np.all(got[-3:] == -7.0)
    if mode == 1:
        assert np.array_equal(got[3:-3], want)
    else:
        assert np.allclose(got[3:-3], want, rtol=1e-6, atol=0)
        report(f"adam statistic sum, {entry}", stat=float((np.abs(got[3:-3] - want) / (1e-6 * np.abs(want))).max()))


# ---------------------------------------------------------------------------------------------------- 4. image loss
@pytest.mark.parametrize("h,w,weight", [(6_657, 161, 0.1), (300, 300, 0.0), (600, 600, 0.0)])
def test_loss_beyond_one_finishing_trip(gpu, h, w, weight):
    """More partial sums than loss_finish_kernel's 256 threads take in one trip, with the generator, assertions and
    tolerances of test_gpu_train.test_loss_matches_oracle:
    6657 x 161, SSIM: ceil(483 / 482) x ceil(6657 / 52) = 2 x 129 = 258 workgroups, the smallest image with a second trip;
    300 x 300, L1 alone: 270,000 elements = 264 workgroups of 1024 elements;
    600 x 600, L1 alone: 1,080,000 elements on the capped grid of 1024 workgroups, more than four trips per thread."""
    from gs_train import ImageLoss

    if weight > 0:
        partials = -(-3 * w // LOSS_FCW) * -(-h // LOSS_SH)
        assert partials == LOSS_FINISH_TRIP + 2
    else:
        partials = min(-(-3 * h * w // L1_PER_BLOCK), L1_BLOCKS)
        assert partials > LOSS_FINISH_TRIP and (partials < L1_BLOCKS or 3 * h * w > L1_BLOCKS * L1_PER_BLOCK)
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    y = np.clip(x + rng.normal(0, 0.1, x.shape), 0, 1).astype(np.float32)
    y[::7, ::5] = x[::7, ::5]  # exact ties: sign(0) = 0
    loss = ImageLoss(h, w, weight, gpu)
    g = loss(dev(x, gpu), dev(y, gpu))
    lo, l1, ssim, grad = train_ref.l1_ssim_loss(x, y, weight)
    vals = loss.values.cpu().numpy()
    err = np.abs(g.cpu().numpy() - grad).max()
    report(f"loss {h}x{w} ssim_weight {weight}, {partials} partial sums", loss=abs(vals[0] - lo) / 2e-6,
           l1=abs(vals[1] - l1) / 1e-6, ssim=abs(vals[2] - ssim) / 2e-6, grad=err / (2e-5 * np.abs(grad).max()))
    assert abs(vals[1] - l1) < 1e-6 and abs(vals[2] - ssim) < 2e-6 and abs(vals[0] - lo) < 2e-6
    assert err < 2e-5 * np.abs(grad).max(), (err, np.abs(grad).max())
