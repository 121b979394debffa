"""GPU tier of the map edit (csrc/map_edit.hip through gs_prune / gs_train.Trainer.prune / Trainer.seed_from_view(carry_state)).

The kernel pair is held against the float32 restatement (tests/prune_ref.py): EQUAL counts and bitwise-equal rows, from a
poisoned workspace into poisoned destinations, twice.  The carried optimizer state is held against its assembly from torch
operations -- the restatement's mask, a plain rebind, moments and statistic set by boolean indexing -- bit for bit, right after
the edit and after one more training step.

Sizes.  The classify grid and the apply grid have one workgroup per 256 rows; the scan is one workgroup with trips of 1,024
counts, so 262,144 + 257 rows cross into its second trip (there is no other boundary: no grid dimension is split)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_prune import opa_logit as opa_logit64, prune_apply, prune_options, prune_rows
from gs_scene import make_camera, make_scene
from gs_seed import seed_from_depth
from gs_testutil import to_torch
from gs_train import TrainOptions, Trainer
from prune_ref import compact, keep_mask, norm, opa_logit

pytestmark = pytest.mark.gpu

OPA_MIN = 0.02
PATTERNS = ("all", "none", "alternating", "last", "r01", "r50", "r99")
RGB5 = (3, 4, 3, 1, 3)
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4099, 262_144 + 257]


def _kept_pattern(n, pattern, g):
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "alternating":
        return np.arange(n) % 2 == 0
    if pattern == "last":
        k = np.zeros(n, bool)
        k[-1:] = True
        return k
    return g.uniform(size=n) >= {"r01": 0.01, "r50": 0.5, "r99": 0.99}[pattern]


def _inputs(n, pattern, widths, act, scale_max, seed, nans=False):
    """scale [n,3], opa [n] and one array per width (scale and opa are arrays 2 and 3 of the rgb layouts).  The opacity decides
    the pattern; a finite scale_max removes some rows more.  No opa equals the threshold, and under exp no norm lies within a
    relative 1e-5 of scale_max: generated so, and asserted."""
    g = np.random.default_rng(seed)
    t = opa_logit(OPA_MIN)
    kept = _kept_pattern(n, pattern, g)
    opa = np.where(kept, t + g.uniform(0.5, 3.0, n), t - g.uniform(0.5, 3.0, n)).astype(np.float32)
    scale = (g.normal(0.0, 0.3, (n, 3)) if act == "abs" else g.normal(-1.0, 0.5, (n, 3))).astype(np.float32)
    if act == "exp" and math.isfinite(scale_max):
        near = np.abs(norm(scale, act) / np.float32(scale_max) - 1.0) <= 1e-4
        scale[near] -= np.float32(0.05)
    if nans and n:
        opa[g.integers(0, n, max(n // 50, 1))] = np.nan
        scale[g.integers(0, n, max(n // 50, 1)), g.integers(0, 3, max(n // 50, 1))] = np.nan
    assert not (opa == t).any()
    if act == "exp" and math.isfinite(scale_max):
        with np.errstate(invalid="ignore"):
            assert not (np.abs(norm(scale, act) / np.float32(scale_max) - 1.0) <= 1e-5).any()
    arrays = []
    for k, w in enumerate(widths):
        if len(widths) >= 5 and k == 2:
            arrays.append(scale)
        elif len(widths) >= 5 and k == 3:
            arrays.append(opa)
        else:
            arrays.append(g.normal(size=(n, w) if w > 1 else (n,)).astype(np.float32))
    return scale, opa, arrays


def _poison(shape, dev):
    """float32 rows of 0xFF bytes."""
    count = int(np.prod(shape)) if len(shape) else 1
    return torch.full((count * 4,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32).view(shape)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _kernel(dev, scale, opa, arrays, act, scale_max, dst_offset=0, short=0, tail=2):
    """classify on a poisoned workspace, apply into poisoned destinations of dst_offset + kept + tail rows with capacity
    dst_offset + kept - short -> ((kept, removed), destination bits)."""
    n = int(scale.shape[0])
    t_scale, t_opa = torch.from_numpy(scale).to(dev), torch.from_numpy(opa).to(dev)
    t_arrays = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    opts = prune_options(OPA_MIN, scale_max, act)
    ws = torch.full((int(_lib.gs_prune_workspace_bytes(n)),), 0xFF, dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    _lib.check(_lib.gs_prune_classify(t_scale.data_ptr(), t_opa.data_ptr(), n, C.byref(opts), counts.data_ptr(), ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream().cuda_stream), "gs_prune_classify")
    kept, removed = (int(v) for v in counts.tolist())
    rows = dst_offset + kept + tail
    dst = [_poison((rows,) + a.shape[1:], dev) for a in arrays]
    prune_apply(t_arrays, dst, n, counts, ws, dst_offset=dst_offset, capacity=dst_offset + kept - short)
    return (kept, removed), [_bits(d) for d in dst]


def _check(dev, n, pattern, widths, act, scale_max, seed, nans=False, dst_offset=0, short=0):
    scale, opa, arrays = _inputs(n, pattern, widths, act, scale_max, seed, nans)
    mask = keep_mask(scale, opa, opa_logit(OPA_MIN), scale_max, act)
    want = compact(arrays, mask)
    kept = int(mask.sum())
    first = _kernel(dev, scale, opa, arrays, act, scale_max, dst_offset, short)
    again = _kernel(dev, scale, opa, arrays, act, scale_max, dst_offset, short)
    assert first[0] == again[0] == (kept, n - kept), (n, pattern, act, first[0], (kept, n - kept))
    for k, (a, b, w) in enumerate(zip(first[1], again[1], want)):
        assert np.array_equal(a, b), (n, pattern, k)  # two runs, the same bytes
        assert np.all(a[:dst_offset] == 0xFFFFFFFF) and np.all(a[dst_offset + kept:] == 0xFFFFFFFF), (n, pattern, k)
        body = a[dst_offset:dst_offset + kept]
        if short and kept:  # one row too few: nothing is written, the counts (above) still hold the need
            assert np.all(body == 0xFFFFFFFF), (n, pattern, k)
        else:
            assert np.array_equal(body, np.ascontiguousarray(w).view(np.uint32)), (n, pattern, k)
    return kept


# ------------------------------------------------------------------------------------- 1. kernel against the restatement
@pytest.mark.parametrize("n", SIZES)
def test_prune_matches_the_restatement(gpu, n):
    """Every pattern at every size, the five rgb arrays, abs with scale_max = +inf; both activations with a finite scale_max
    (0.6 for abs, 0.9 for exp: some 70 - 75 % of the generated norms lie below, so the scale test decides too) on two patterns."""
    seen = set()
    for i, pattern in enumerate(PATTERNS):
        kept = _check(gpu, n, pattern, RGB5, "abs", math.inf, seed=1000 * i + n % 997)
        seen.add(kept)
        if pattern in ("all", "r50"):
            for act, smax in (("abs", 0.6), ("exp", 0.9), ("exp", math.inf)):
                k2 = _check(gpu, n, pattern, RGB5, act, smax, seed=1000 * i + n % 997 + 7)
                if n >= 255 and math.isfinite(smax):
                    assert 0.1 * n < k2 < (0.9 if pattern == "all" else 0.45) * n  # the scale test removed rows of its own
    if n >= 255:
        assert {0, n, 1, (n + 1) // 2} <= seen


@pytest.mark.parametrize("widths", [RGB5, RGB5 * 3 + (3,), (1,), (3, 4, 3, 1, 27), (3, 4, 3, 1, 48),
                                    (3, 4, 3, 1, 27) * 3 + (3,), (3, 4, 3, 1, 48) * 3 + (3,)],
                         ids=["rgb5", "rgb16", "w1", "sh27", "sh48", "sh27x16", "sh48x16"])
def test_prune_moves_every_array_set(gpu, widths):
    """The array sets -- five rgb arrays, all sixteen, a single width-1 array, SH degree 2 and 3 colour rows (and sixteen arrays
    with them) -- at 257 rows (two workgroups, the second with one row) and 4,099, half removed and 1 % removed."""
    for n in (257, 4099):
        for pattern in ("r50", "r01", "last"):
            _check(gpu, n, pattern, widths, "abs", math.inf, seed=n + len(widths))


def test_prune_nan_offset_and_capacity(gpu):
    """NaN in opa and in scale (never kept, whatever the thresholds); dst_offset > 0 leaves the rows in front untouched; a
    capacity one short writes nothing while the counts still hold the need."""
    for n in (65, 257, 4099):
        for act, smax in (("abs", math.inf), ("abs", 0.6), ("exp", 0.9)):
            _check(gpu, n, "r50", RGB5, act, smax, seed=n, nans=True)
        for off in (1, 300):
            _check(gpu, n, "r50", RGB5 * 3 + (3,), "abs", math.inf, seed=n + off, dst_offset=off)
            _check(gpu, n, "r01", (3, 4, 3, 1, 27), "abs", 0.6, seed=n + off, dst_offset=off, nans=True)
        _check(gpu, n, "r50", RGB5, "abs", math.inf, seed=n + 1, short=1)
        _check(gpu, n, "all", RGB5 * 3 + (3,), "abs", math.inf, seed=n + 2, dst_offset=5, short=1)


def test_prune_rows_is_the_torch_statement(gpu):
    """The thin wrapper against ``mask = ...; [t[mask] for t in arrays]`` on the device."""
    scale, opa, arrays = _inputs(4099, "r50", RGB5 * 3 + (3,), "abs", 0.6, seed=5)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]
    out, kept, removed = prune_rows(t[2], t[3], t, opa_min=OPA_MIN, scale_max=0.6, scale_activation="abs")
    mask = (t[3] > float(opa_logit(OPA_MIN))) & (t[2].abs().square().sum(-1).sqrt() < 0.6)
    assert kept == int(mask.sum()) and kept + removed == 4099 and 0 < kept < 2000
    for o, a in zip(out, t):
        assert torch.equal(o, a[mask])
    out0, kept0, removed0 = prune_rows(t[2][:0], t[3][:0], [a[:0] for a in t], opa_min=OPA_MIN, scale_max=None)
    assert (kept0, removed0) == (0, 0) and all(o.shape[0] == 0 for o in out0)


# ------------------------------------------------------------------------------------------------------------ 2. Trainer
_VIEWS = {}


def _views(gpu, W=160, H=112):
    """The scene of tests/test_gpu_seed.py::_views: a small make_scene truth, colour targets rendered from it, range targets
    D / A where A >= 0.9 (0 elsewhere), three views that overlap only partly.  Built once."""
    if not _VIEWS:
        scene = make_scene(6_000, W, H, seed=31)
        cams = []
        for yaw, tx in ((0.0, 0.0), (-16.0, -0.5), (16.0, 0.5)):
            c = make_camera(W, H, yaw_deg=yaw)
            c.tran = np.array([tx, 0.0, 0.0], np.float32)
            cams.append(c)
        gt = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=True)
        images, ranges = [], []
        for cam in cams:
            img, _, d, a = r.forward(*gt, cam, training=False, aux=True)
            images.append(img.clamp(0, 1).clone())
            ranges.append(torch.where(a >= 0.9, d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous())
        _VIEWS["x"] = (cams, images, ranges, seed_from_depth(images[0], ranges[0], cams[0]))
    return _VIEWS["x"]


def _trainer(gpu, steps=4, **kw):
    """The trainer of tests/test_gpu_seed.py::_trainer on the seeds of view 0, ``steps`` steps on views 0, 1, 2, 0, ... in."""
    cams, images, ranges, start = _views(gpu)
    opt = TrainOptions(n_iters=51, n_iters_warmup=5, depth_weight=0.2)
    tr = Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 21, depths=ranges, **kw)
    for i in range(steps):
        tr.train_step(i, i % 3)
    return tr


def _state(tr):
    o = tr.optimizer
    return [tr.flat.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.accum_grad.clone()]


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(_state(a), _state(b))) \
        and a.optimizer.step_count == b.optimizer.step_count


NAMES = ("pos", "quat", "scale", "opa", "rgb")


def test_trainer_prune_carries_the_optimizer_state(gpu):
    a, b, c = _trainer(gpu), _trainer(gpu), _trainer(gpu)
    assert _same(a, b) and _same(a, c) and a.optimizer.exp_avg.abs().max() > 0 and a.optimizer.accum_grad.abs().max() > 0
    n = a.n_gaussians
    subset = torch.arange(3, n, 7, device=gpu)
    for tr in (a, b, c):
        tr.flat.params[3][subset] = -20.0
    # (a) the kernel path
    flat_a, opt_a = a.flat, a.optimizer
    removed = a.prune(4, opa_min=0.005)
    assert removed == subset.numel() and a.n_gaussians == n - removed and a.flat is not flat_a and a.optimizer is not opt_a
    # (b) the torch assembly: the restatement's mask, a plain rebind, moments and statistic by boolean indexing
    old = [p.clone() for p in b.flat.params]
    mask_np = keep_mask(old[2].cpu().numpy(), old[3].cpu().numpy(), opa_logit(0.005), np.inf, "abs")
    assert int((~mask_np).sum()) == subset.numel()
    mask = torch.from_numpy(mask_np).to(gpu)
    moments = {name: [m.clone() for m in b.optimizer.moment_rows(name)] for name in NAMES}
    stat, steps = b.optimizer.accum_grad.clone(), b.optimizer.step_count
    b._bind([p[mask] for p in old], 4)
    for name in NAMES:
        for dst, src in zip(b.optimizer.moment_rows(name), moments[name]):
            dst.copy_(src[mask])
    b.optimizer.accum_grad.copy_(stat[mask])
    b.optimizer.step_count = steps
    assert steps == 4 and _same(a, b)
    pruned_params = a.flat.flat_param.clone()
    la, lb = a.train_step(4, 1).clone(), b.train_step(4, 1).clone()
    assert _same(a, b) and torch.equal(la, lb) and a.optimizer.step_count == 5
    assert not torch.equal(a.flat.flat_param, pruned_params)  # (the step moved the parameters)
    # a prune that removes nothing changes nothing: the same optimizer object, the same flat buffer
    flat_a, opt_a, before = a.flat, a.optimizer, _state(a)
    assert a.prune(5, opa_min=1e-9) == 0 and a.flat is flat_a and a.optimizer is opt_a
    assert all(torch.equal(x, y) for x, y in zip(before, _state(a)))
    # carry_state=False: the same rows, the fresh optimizer of every other rebind
    assert c.prune(4, opa_min=0.005, carry_state=False) == removed
    assert torch.equal(c.flat.flat_param, pruned_params) and c.optimizer.step_count == 0
    assert not c.optimizer.exp_avg.any() and not c.optimizer.exp_avg_sq.any() and not c.optimizer.accum_grad.any()
    # pad rows stay zero
    for name in NAMES:
        _, hi = a.flat.offsets[name]
        end = a.flat.region[name] + a.flat.n_pad * a.flat.width[name]
        assert not pruned_params[hi:end].any()
    with pytest.raises(RuntimeError, match="all"):
        c.prune(5, opa_min=0.999999)


def test_trainer_seed_from_view_carries_the_optimizer_state(gpu):
    a, b = _trainer(gpu), _trainer(gpu)
    n_old = a.n_gaussians
    moments = {name: [m.clone() for m in b.optimizer.moment_rows(name)] for name in NAMES}
    stat, steps = b.optimizer.accum_grad.clone(), b.optimizer.step_count
    added = a.seed_from_view(1, 4, carry_state=True)
    assert added > 0 and b.seed_from_view(1, 4) == added  # (b): the fresh rebind, then the state put back by hand
    assert b.optimizer.step_count == 0 and not b.optimizer.exp_avg.any()
    for name in NAMES:
        for dst, src in zip(b.optimizer.moment_rows(name), moments[name]):
            dst[:n_old].copy_(src)
    b.optimizer.accum_grad[:n_old].copy_(stat)
    b.optimizer.step_count = steps
    assert _same(a, b) and a.optimizer.step_count == 4 and a.n_gaussians == n_old + added
    for name in NAMES:  # old rows bitwise what they were, new rows zero
        for got, src in zip(a.optimizer.moment_rows(name), moments[name]):
            assert torch.equal(got[:n_old], src) and not got[n_old:].any()
    assert torch.equal(a.optimizer.accum_grad[:n_old], stat) and not a.optimizer.accum_grad[n_old:].any()
    # nothing selected (the view is explained now): nothing changes, no rebind
    flat, opt_, before = a.flat, a.optimizer, _state(a)
    assert a.seed_from_view(1, 4, carry_state=True) == 0 and a.flat is flat and a.optimizer is opt_
    assert all(torch.equal(x, y) for x, y in zip(before, _state(a))) and a.optimizer.step_count == 4
    la, lb = a.train_step(4, 1).clone(), b.train_step(4, 1).clone()
    assert _same(a, b) and torch.equal(la, lb) and a.optimizer.step_count == 5


def test_carrying_is_refused_where_the_moments_are_not_row_addressable(gpu):
    """A sharded optimizer, several ranks, a per-view statistic: RuntimeError before anything changes; without carry_state
    the same calls run as any rebind."""
    for kw in ({"exchange": "reduce_scatter"}, {"per_view_stat": True, "densify": True}, {"world": 2}):
        world = kw.pop("world", None)
        tr = _trainer(gpu, steps=2, **kw)
        if world:
            tr.world_size = world
        tr.flat.params[3][::5] = -20.0
        flat, opt_, before = tr.flat, tr.optimizer, tr.flat.flat_param.clone()
        with pytest.raises(RuntimeError, match="carry_state=False"):
            tr.prune(2, opa_min=0.005)
        with pytest.raises(RuntimeError, match="carry_state=False"):
            tr.seed_from_view(1, 2, carry_state=True)
        assert tr.flat is flat and tr.optimizer is opt_ and torch.equal(tr.flat.flat_param, before)
        if world:
            tr.world_size = 1
        n = tr.n_gaussians
        assert tr.prune(2, opa_min=0.005, carry_state=False) == len(range(0, n, 5)) and tr.optimizer.step_count == 0


def test_pruning_transparent_gaussians_leaves_the_image(gpu):
    """Rows whose opacity logit is -20 (alpha <= 2.1e-9) contribute nothing the renderer keeps: the view rendered before and
    after pruning them agrees within the project's image tolerance, 5e-5 (README, parity).  Printed: whether bitwise.
    Measured on an MI355X (profiles/prune_cost.txt): max |diff| 1.8e-7, not bitwise."""
    cams, images, ranges, start = _views(gpu)
    params = [t.clone() for t in start]
    params[3][::3] = -20.0
    r = FrameRenderer(gpu, max_pairs=1 << 21, auto_grow=True)
    before = r.forward(*params, cams[0], training=False)[0].clone()
    out, kept, removed = prune_rows(params[2], params[3], params, opa_min=0.005, scale_max=None, scale_activation="abs")
    assert removed == len(range(0, params[0].shape[0], 3)) and opa_logit64(0.005) > -20.0
    after = r.forward(*out, cams[0], training=False)[0]
    err = float((after - before).abs().max())
    print(f"prune of {removed} rows at logit -20 out of {kept + removed}: image max |diff| {err:.3e} "
          f"({'bitwise equal' if torch.equal(after, before) else 'not bitwise equal'})")
    assert err <= 5e-5
