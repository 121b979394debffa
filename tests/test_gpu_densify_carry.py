"""GPU tier of the carried densification (csrc/densify.hip: gs_densify_apply_state, through gs_densify.densify_apply_state and
gs_train.Trainer.adaptive_control(carry_state=True)).

The kernel is held against the numpy restatement (tests/densify_carry_ref.py) bit for bit, into destinations that hold a NaN
pattern, twice, in both orders with gs_densify_apply.  The Trainer's carried state is held against its assembly from torch
operations -- a plain adaptive_control, the moments put back by boolean indexing from the restatement's classes -- bit for bit,
right after the edit and after one more training step.

Sizes.  The classify grid and both apply grids have one workgroup per 256 rows; the scan is one workgroup with trips of 1,024
counts, so row 262,144 is the first of its second trip (there is no other boundary: no grid dimension is split)."""
import numpy as np
import pytest
import torch

from densify_carry_ref import CLONE, DELETE, KEEP, SPLIT, apply_state, classes, counts as class_counts
from gs_densify import (adaptive_control, densify_apply, densify_apply_state, densify_classify, inverse_sigmoid)
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_seed import seed_from_depth
from gs_testutil import to_torch
from gs_train import TrainOptions, Trainer
from oracle import densify_ref
from test_gpu_densify import random_set
from test_gpu_step_regimes import DENSIFY_ONE_TRIP, oracle_classes

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF  # a quiet NaN that no computation here produces
RGB5, SH27, SH48 = (3, 4, 3, 1, 3), (3, 4, 3, 1, 27), (3, 4, 3, 1, 48)
WIDTH_SETS = {"rgb10": RGB5 * 2, "sh27x10": SH27 * 2, "sh48x10": SH48 * 2, "w1": (1,), "rgb16": RGB5 * 3 + (3,)}
TAIL = 3  # destination rows behind the total


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _pattern(shape, gpu):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=gpu).view(torch.float32)


def _state_arrays(n, widths, seed):
    g = np.random.default_rng(seed)
    return [g.normal(size=(n, w) if w > 1 else (n,)).astype(np.float32) for w in widths]


class _Set:
    """A random_set on the device, classified once: the tensors, the restatement's classes, the device's counts."""

    def __init__(self, gpu, n, act, use_clone=True, use_split=True):
        arrays, grad, draws = random_set(n, 3, act)
        self.n, self.kw = n, dict(scale_activation=act, grad_aggregation="max", use_clone=use_clone, use_split=use_split)
        self.cls = classes(arrays[2], arrays[3], grad, act, "max", use_clone, use_split)
        assert np.array_equal(self.cls, oracle_classes(arrays, grad, act, "max", use_clone, use_split))
        want = densify_ref.adaptive_control(*arrays, grad, 0.05, 0.17, *draws, **self.kw)[5]
        assert class_counts(self.cls) == want  # the classes are the oracle's decision
        self.params, self.grad = [_dev(a, gpu) for a in arrays], _dev(grad, gpu)
        self.draws = tuple(_dev(d, gpu) for d in draws)
        self.counts, self.ws, self.opts = densify_classify(self.params, self.grad, 0.05, 0.17, **self.kw)
        self.kcs = tuple(int(v) for v in self.counts.tolist())
        assert self.kcs[:3] == want and self.kcs[3] == sum(want)
        self.total = self.kcs[3]

    def state(self, gpu, src, capacity=None):
        """One gs_densify_apply_state into destinations that hold the pattern, TAIL rows longer than the total."""
        dst = [_pattern((self.total + TAIL,) + tuple(s.shape[1:]), gpu) for s in src]
        densify_apply_state(src, dst, self.n, self.counts, self.ws, capacity=self.total if capacity is None else capacity)
        return [_bits(d) for d in dst]

    def apply(self, gpu):
        out = [torch.empty((self.total,) + tuple(t.shape[1:]), dtype=torch.float32, device=gpu) for t in self.params]
        densify_apply(self.params, self.grad, out, self.counts, self.ws, self.opts, self.draws, self.kcs[2], self.total)
        return [_bits(o) for o in out]


def _check_state(gpu, s, widths, seed):
    arrays = _state_arrays(s.n, widths, seed)
    want = apply_state(s.cls, arrays)
    src = [_dev(a, gpu) for a in arrays]
    first, again = s.state(gpu, src), s.state(gpu, src)
    for k, (a, b, w) in enumerate(zip(first, again, want)):
        assert np.array_equal(a, b), (s.n, k)  # two calls, the same bytes
        body, tail = a[:s.total], a[s.total:]
        assert w.shape[0] == s.total and len(tail) == TAIL and np.all(tail == NAN_BITS), (s.n, k)
        assert not np.any(body == NAN_BITS), (s.n, k)  # every row written
        assert np.array_equal(body, np.ascontiguousarray(w).view(np.uint32)), (s.n, k)  # (a zero is +0: all bits clear)
    if s.total:  # one row too few: nothing is written
        for a in s.state(gpu, src, capacity=s.total - 1):
            assert np.all(a == NAN_BITS)
    return first


# ------------------------------------------------------------------------------------- 1. kernel against the restatement
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_state_matches_the_restatement(gpu, n):
    """Every width set, both activations, clone and split on and off, at a lone row, the workgroup edges and several
    workgroups with a ragged tail."""
    for act in ("abs", "exp"):
        for use_clone, use_split in ((True, True), (False, True), (True, False), (False, False)):
            s = _Set(gpu, n, act, use_clone, use_split)
            k, c, sp = class_counts(s.cls)
            if n >= 255:
                deleted, plain = int((s.cls == DELETE).sum()), int((s.cls == KEEP).sum())
                assert deleted > 0 and plain > 0 and (c > 0) == use_clone and (sp > 0) == use_split, (n, act, k, c, sp)
                assert int((s.cls == CLONE).sum()) == c and int((s.cls == SPLIT).sum()) == sp
            for i, widths in enumerate(WIDTH_SETS.values()):
                _check_state(gpu, s, widths, seed=7 * n + i)


def test_state_beyond_one_scan_trip(gpu):
    """262,145 rows: the last row's workgroup takes its three offsets from the scan's second trip.  The ten rgb moment arrays."""
    n = DENSIFY_ONE_TRIP + 1
    s = _Set(gpu, n, "abs")
    assert min(s.kcs) > 0 and (s.cls == DELETE).any() and (s.cls == KEEP).any()
    _check_state(gpu, s, WIDTH_SETS["rgb10"], seed=n)


@pytest.mark.parametrize("n,act", [(257, "abs"), (1000, "exp")])
def test_state_and_apply_do_not_disturb_each_other(gpu, n, act):
    """gs_densify_apply before or after gs_densify_apply_state: the parameters are adaptive_control's, the state is the same."""
    s = _Set(gpu, n, act)
    alone, counts = adaptive_control(s.params, s.grad, 0.05, 0.17, draws=s.draws, **s.kw)
    assert counts == s.kcs[:3]
    alone = [_bits(t) for t in alone]
    src = [_dev(a, gpu) for a in _state_arrays(n, WIDTH_SETS["rgb10"], seed=n)]
    params_first = s.apply(gpu)
    state_after = s.state(gpu, src)
    s2 = _Set(gpu, n, act)
    state_before = s2.state(gpu, src)
    params_second = s2.apply(gpu)
    for a, b, w in zip(params_first, params_second, alone):
        assert np.array_equal(a, w) and np.array_equal(b, w)
    for a, b in zip(state_after, state_before):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 2. Trainer
_VIEWS = {}
NAMES = ("pos", "quat", "scale", "opa", "rgb")


def _views(gpu, W=160, H=112):
    """The scene of tests/test_gpu_prune.py::_views, rebuilt here: a small make_scene truth, colour targets rendered from it,
    range targets D / A where A >= 0.9 (0 elsewhere), three views that overlap only partly.  Built once."""
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


def _build(gpu, opt=None, seed=11, **kw):
    cams, images, ranges, start = _views(gpu)
    opt = opt or TrainOptions(n_iters=51, n_iters_warmup=5, depth_weight=0.2, use_clone=1, use_split=1)
    kw.setdefault("densify", True)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(seed)
    return Trainer([t.clone() for t in start], cams, images, opt, max_pairs=1 << 21, depths=ranges, generator=gen, **kw)


def _trainer(gpu, steps=4, **kw):
    """The trainer of tests/test_gpu_prune.py::_trainer with densify=True and a seeded generator, ``steps`` steps on views
    0, 1, 2, 0, ... in (the default schedule's first control iteration lies far behind them)."""
    tr = _build(gpu, **kw)
    for i in range(steps):
        tr.train_step(i, i % 3)
    return tr


def _state(tr):
    o = tr.optimizer
    return [tr.flat.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.accum_grad.clone()]


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in zip(_state(a), _state(b))) and a.optimizer.step_count == b.optimizer.step_count


def _between(sorted_values, q):
    """A threshold between two neighbouring values at quantile q: no row sits on it."""
    i = int(q * (len(sorted_values) - 1))
    return 0.5 * (float(sorted_values[i]) + float(sorted_values[i + 1]))


def test_trainer_adaptive_control_carries_the_moments(gpu):
    a, b, c = _trainer(gpu), _trainer(gpu), _trainer(gpu)
    assert _same(a, b) and _same(a, c) and a.optimizer.exp_avg.abs().max() > 0 and a.optimizer.accum_grad.abs().max() > 0
    n = a.n_gaussians
    subset = torch.arange(3, n, 7, device=gpu)
    for tr in (a, b, c):
        tr.flat.params[3][subset] = -20.0
    # thresholds from the scene itself, so that every class occurs: the largest 3 % go, half of the rest counts as large, half
    # as moving -- each threshold between two neighbouring values
    scale = a.flat.params[2].detach().cpu().numpy()
    opa = a.flat.params[3].detach().cpu().numpy()
    stat = (a.optimizer.accum_grad / (1.0 + 1e-3)).cpu().numpy()  # train.py:160 as Trainer.adaptive_control states it
    norm = np.sort(np.sqrt((np.abs(scale) ** 2).sum(-1, dtype=np.float32)))
    agg = np.sort(np.abs(stat).max(-1))
    thresholds = dict(split_thresh=_between(norm, 0.5), delete_thresh=_between(norm, 0.97), grad_thresh=_between(agg, 0.5))
    for tr in (a, b, c):
        for key, v in thresholds.items():
            setattr(tr.opt, key, v)
    cls = classes(scale, opa, stat, "abs", "max", True, True, taus=thresholds["split_thresh"],
                  delete_thresh=thresholds["delete_thresh"], grad_thresh=thresholds["grad_thresh"])
    K, C, S = class_counts(cls)
    deleted, plain = int((cls == DELETE).sum()), int((cls == KEEP).sum())
    assert deleted >= subset.numel() and plain > 0 and C > 0 and S > 0 and deleted + K == n
    # (a) the kernel path
    flat_a, opt_a = a.flat, a.optimizer
    assert a.adaptive_control(4, carry_state=True) == (K, C, S)
    assert a.n_gaussians == K + C + S and a.flat is not flat_a and a.optimizer is not opt_a
    # (b) the torch assembly: a plain adaptive_control, then the moments by boolean indexing from the restatement's classes
    moments = {name: [m.clone() for m in b.optimizer.moment_rows(name)] for name in NAMES}
    steps = b.optimizer.step_count
    assert b.adaptive_control(4, carry_state=False) == (K, C, S)
    assert b.optimizer.step_count == 0 and not b.optimizer.exp_avg.any() and not b.optimizer.exp_avg_sq.any()
    kept = torch.from_numpy(cls != DELETE).to(gpu)
    split_slot = torch.from_numpy(cls[cls != DELETE] == SPLIT).to(gpu)
    for name in NAMES:
        for dst, src in zip(b.optimizer.moment_rows(name), moments[name]):
            rows = src[kept].clone()
            rows[split_slot] = 0
            dst[:K].copy_(rows)
    b.optimizer.step_count = steps
    # (c) carry_state=False, left alone
    assert c.adaptive_control(4, carry_state=False) == (K, C, S)
    assert steps == 4 and _same(a, b) and a.optimizer.step_count == 4
    for x, y in ((a, b), (a, c)):  # the parameters do not depend on carrying: not one bit
        assert torch.equal(x.flat.flat_param.view(torch.int32), y.flat.flat_param.view(torch.int32))
    assert not a.optimizer.accum_grad.any()  # the statistic has been consumed
    assert c.optimizer.step_count == 0 and not c.optimizer.exp_avg.any() and not c.optimizer.exp_avg_sq.any()
    assert not c.optimizer.accum_grad.any()
    # what travelled: kept and cloned rows carry moments, split slots and the new rows do not
    m, v = a.optimizer.moment_rows("pos")
    assert m[:K][~split_slot].abs().max() > 0 and v[:K][~split_slot].abs().max() > 0
    assert not m[:K][split_slot].any() and not m[K:].any() and not v[K:].any()
    # pad rows stay zero, in the parameters and in both moments
    for buf in (a.flat.flat_param, a.optimizer.exp_avg, a.optimizer.exp_avg_sq):
        for name in NAMES:
            _, hi = a.flat.offsets[name]
            end = a.flat.region[name] + a.flat.n_pad * a.flat.width[name]
            assert not buf[hi:end].any()
    edited = a.flat.flat_param.clone()
    la, lb = a.train_step(4, 1).clone(), b.train_step(4, 1).clone()
    assert _same(a, b) and torch.equal(la, lb) and a.optimizer.step_count == 5
    assert not torch.equal(a.flat.flat_param, edited)  # (the step moved the parameters)


def test_only_delete_path_carries_too(gpu):
    """densify=False: no clones, no splits -- the kept rows keep their moments in order (what Trainer.prune would carry)."""
    a, b = _trainer(gpu), _trainer(gpu)
    n = a.n_gaussians
    subset = torch.arange(3, n, 7, device=gpu)
    for tr in (a, b):
        tr.flat.params[3][subset] = -20.0
    moments = {name: [m.clone() for m in a.optimizer.moment_rows(name)] for name in NAMES}
    cls = classes(a.flat.params[2].detach().cpu().numpy(), a.flat.params[3].detach().cpu().numpy(),
                  (a.optimizer.accum_grad / (1.0 + 1e-3)).cpu().numpy(), "abs", "max", False, False,
                  taus=a.opt.split_thresh, delete_thresh=a.opt.delete_thresh, grad_thresh=a.opt.grad_thresh)
    K = int((cls != DELETE).sum())
    assert 0 < K <= n - subset.numel()
    assert a.adaptive_control(4, densify=False, carry_state=True) == (K, 0, 0)
    assert b.adaptive_control(4, densify=False, carry_state=False) == (K, 0, 0)
    assert torch.equal(a.flat.flat_param.view(torch.int32), b.flat.flat_param.view(torch.int32))
    kept = torch.from_numpy(cls != DELETE).to(gpu)
    for name in NAMES:
        for got, src in zip(a.optimizer.moment_rows(name), moments[name]):
            assert torch.equal(got.view(torch.int32), src[kept].view(torch.int32))
    assert a.optimizer.step_count == 4 and b.optimizer.step_count == 0 and a.n_gaussians == K


def test_the_schedule_carries_when_the_trainer_is_built_so(gpu):
    """Trainer(densify_carry=True) on a schedule whose iteration 3 is a control iteration: the step count goes on through it;
    the default Trainer restarts it there."""
    def options():
        return TrainOptions(n_iters=51, n_iters_warmup=5, depth_weight=0.2, adaptive_control_start_iter=1,
                            n_adaptive_control=3, grad_accum_iters=2)

    carried, default = _build(gpu, options(), densify_carry=True), _build(gpu, options())
    assert carried.densify_carry is True and default.densify_carry is False
    for tr in (carried, default):
        assert [tr._is_control_iteration(i) for i in range(5)] == [False, False, False, True, False]
        for i in range(3):
            tr.train_step(i, i % 3)
    flat_c, flat_d = carried.flat, default.flat
    for tr in (carried, default):
        tr.train_step(3, 0)
        tr.train_step(4, 1)
    assert carried.flat is not flat_c and default.flat is not flat_d  # both went through adaptive_control
    assert carried.n_gaussians == default.n_gaussians > 0
    assert carried.optimizer.step_count == 5 and default.optimizer.step_count == 1


def test_opacity_reset_zeroes_the_opacity_moments_under_carry(gpu):
    """Twin densify_carry trainers that differ only in n_opa_reset: after the reset iteration every opacity logit of the first
    is logit(0.01) and both its opa moment views are zero; its other eight moment arrays are the twin's, bit for bit.  Without
    densify_carry the same reset leaves the opacity moments alone."""
    def options(n_opa_reset):
        return TrainOptions(n_iters=51, n_iters_warmup=5, depth_weight=0.2, n_opa_reset=n_opa_reset)

    first, twin = _build(gpu, options(3), densify_carry=True), _build(gpu, options(10_000_000), densify_carry=True)
    plain = _build(gpu, options(3))
    for i in range(4):
        for tr in (first, twin, plain):
            tr.train_step(i, i % 3)
    logit = torch.tensor(inverse_sigmoid(0.01), dtype=torch.float32, device=gpu)
    assert torch.equal(first.flat.params[3], logit.expand_as(first.flat.params[3]))
    assert torch.equal(plain.flat.params[3], first.flat.params[3]) and not torch.equal(twin.flat.params[3], first.flat.params[3])
    for m in first.optimizer.moment_rows("opa"):
        assert not m.any()
    for m_twin, m_plain in zip(twin.optimizer.moment_rows("opa"), plain.optimizer.moment_rows("opa")):
        assert m_twin.abs().max() > 0 and torch.equal(m_twin, m_plain)
    for name in ("pos", "quat", "scale", "rgb"):
        for x, y in zip(first.optimizer.moment_rows(name), twin.optimizer.moment_rows(name)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and x.abs().max() > 0
    assert first.optimizer.step_count == twin.optimizer.step_count == 4


def test_carrying_is_refused_where_the_moments_are_not_row_addressable(gpu):
    """A sharded optimizer and several ranks: RuntimeError before anything changes, at construction with densify_carry=True
    and at adaptive_control(carry_state=True); with carry_state=False the same trainers run."""
    with pytest.raises(RuntimeError, match="carry_state=False"):
        _build(gpu, exchange="reduce_scatter", densify_carry=True)
    with pytest.raises(RuntimeError, match="carry_state=False"):
        _build(gpu, world_size=2, densify_carry=True)
    for kw in ({"exchange": "reduce_scatter"}, {"world": 2}):
        world = kw.pop("world", None)
        tr = _trainer(gpu, steps=2, **kw)
        if world:
            tr.world_size = world
        tr.flat.params[3][::5] = -20.0
        flat, opt_, before = tr.flat, tr.optimizer, tr.flat.flat_param.clone()
        stat, steps = tr.optimizer.accum_grad.clone(), tr.optimizer.step_count
        with pytest.raises(RuntimeError, match="carry_state=False"):
            tr.adaptive_control(2, carry_state=True)
        assert tr.flat is flat and tr.optimizer is opt_ and torch.equal(tr.flat.flat_param, before)
        assert torch.equal(tr.optimizer.accum_grad, stat) and tr.optimizer.step_count == steps == 2
        if world:
            tr.world_size = 1
        n = tr.n_gaussians
        kept, cloned, split = tr.adaptive_control(2, carry_state=False)
        assert 0 < kept <= n - len(range(0, n, 5)) and tr.optimizer.step_count == 0
        assert tr.n_gaussians == kept + cloned + split
