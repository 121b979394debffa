#!/usr/bin/env python3
"""What carrying Adam's moments through a densification costs.

    python tools/densify_carry_cost.py [--blocks 9] [--calls 20]

1. ``Trainer.adaptive_control`` with carry_state off and on -- the whole control step as the fit pays it: classify, the host
   read of the counts, the draws, the rebind (new flat buffer, new optimizer), the apply launch(es) -- at 376 k and 2.4 M rows,
   rgb and SH degree 2 colours.  One call per block and arm, device events around it, the Trainer put back to the same start
   state (untimed) before each; the two arms interleaved block by block; median (min .. max).
2. The state launch alone (gs_densify_apply_state, the ten moment arrays), blocks of back-to-back calls between two events,
   interleaved with gs_prune_apply moving the SAME ten arrays under the same delete rule (logit(0.02), ||scale|| < delete_thresh:
   the same kept rows) -- the project's own figure for this kind of kernel (profiles/prune_cost.txt).  Bytes: rows read + rows
   written + the per-row decision the kernel reads (4 bytes of class; an eighth of a byte of ballot for the prune).
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import torch  # noqa: E402

from gs_densify import densify_apply_state, densify_classify  # noqa: E402
from gs_prune import prune_apply, prune_classify, prune_options  # noqa: E402
from gs_scene import make_camera  # noqa: E402
from gs_train import TrainOptions, Trainer  # noqa: E402

NAMES = ("pos", "quat", "scale", "opa", "rgb")
# thresholds of tests/test_gpu_densify.py's random sets: every class occurs (about a quarter deleted, a tenth kept as they
# are, 2 % cloned, the rest split)
OPT = dict(split_thresh=0.05, delete_thresh=0.17, grad_thresh=0.0002, use_clone=1, use_split=1)


def make_set(n, color_dim, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    scale = (0.005 + 0.115 * u(n, 3)) * torch.where(u(n, 3) < 0.5, -1.0, 1.0)
    params = [r(n, 3), r(n, 4), scale, -2.0 + 2.5 * r(n), r(n, color_dim)]
    stat = (r(n, 3) * 3e-4).abs()
    moments = [(r(*p.shape) * 1e-3, u(*p.shape) * 1e-6) for p in params]
    return params, stat, moments


def event_time(fn, calls=1):
    tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tic.record()
    for _ in range(calls):
        fn()
    toc.record()
    toc.synchronize()
    return tic.elapsed_time(toc) * 1000.0 / calls


def fmt(v):
    return f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    cam = make_camera(64, 48)
    target = torch.zeros(48, 64, 3, device=dev)
    print(f"densify_carry cost: microseconds, median (min .. max) over {a.blocks} interleaved blocks")
    for n in (376_000, 2_400_000):
        for color_dim, cname in ((3, "rgb"), (27, "SH degree 2")):
            params, stat, moments = make_set(n, color_dim, dev, seed=n % 1000 + color_dim)
            tr = Trainer([p.clone() for p in params], [cam], [target], TrainOptions(**OPT), max_pairs=1 << 16, densify=True,
                         generator=torch.Generator(device=dev).manual_seed(1))

            def reset():
                tr._bind(params, 0)
                tr.optimizer.accum_grad.copy_(stat)
                tr.optimizer.step_count = 100
                for name, (m, v) in zip(NAMES, moments):
                    dm, dv = tr.optimizer.moment_rows(name)
                    dm.copy_(m)
                    dv.copy_(v)
                torch.cuda.synchronize()

            times, result = {False: [], True: []}, {}
            for block in range(-2, a.blocks):  # two warm-up blocks
                for carry in (False, True):
                    reset()
                    t = event_time(lambda: result.__setitem__(carry, tr.adaptive_control(100, carry_state=carry)))
                    if block >= 0:
                        times[carry].append(t)
            assert result[False] == result[True]
            K, C, S = result[True]
            row_bytes = 4 * (3 + 4 + 3 + 1 + color_dim)
            print(f"{n} rows, {cname} ({row_bytes} B of parameters per row): kept {K} (of them split {S}), cloned {C}, "
                  f"new set {K + C + S}")
            print(f"    Trainer.adaptive_control, fresh Adam    {fmt(times[False])}")
            print(f"    Trainer.adaptive_control, carry_state   {fmt(times[True])}")
            print(f"    carry_state - fresh: {statistics.median(times[True]) - statistics.median(times[False]):+.1f} us")
            # ---- the state launch alone, beside gs_prune_apply on the same ten arrays
            reset()
            src = [t for name in NAMES for t in tr.optimizer.moment_rows(name)]
            counts, ws, _ = densify_classify([p.detach() for p in tr.flat.params], stat / (1.0 + 1e-3), OPT["split_thresh"],
                                             OPT["delete_thresh"], "abs", OPT["grad_thresh"], "max", True, True)
            assert tuple(counts.tolist()[:3]) == (K, C, S)
            total = K + C + S
            dst = [torch.empty((total,) + tuple(t.shape[1:]), device=dev) for t in src]
            p_counts, p_ws = prune_classify(tr.flat.params[2].detach(), tr.flat.params[3].detach(),
                                            prune_options(0.02, OPT["delete_thresh"], "abs"))
            assert p_counts.tolist()[0] == K, "the prune's delete rule keeps other rows"
            p_dst = [torch.empty((K,) + tuple(t.shape[1:]), device=dev) for t in src]
            fns = (("gs_densify_apply_state", lambda: densify_apply_state(src, dst, n, counts, ws, capacity=total)),
                   ("gs_prune_apply", lambda: prune_apply(src, p_dst, n, p_counts, p_ws, capacity=K)))
            for _, fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            launch = {label: [] for label, _ in fns}
            for _ in range(a.blocks):
                for label, fn in fns:
                    launch[label].append(event_time(fn, a.calls))
            # two moments per parameter array: 2 x row_bytes per row.  The state launch reads the K - S rows that keep their
            # moments and writes the whole new set; the prune reads and writes the K kept rows
            moved = {"gs_densify_apply_state": 2 * row_bytes * ((K - S) + total) + 4 * n,
                     "gs_prune_apply": 2 * row_bytes * 2 * K + n // 8}
            for label, _ in fns:
                med = statistics.median(launch[label])
                print(f"    {label:24s} alone, ten moment arrays {fmt(launch[label])}   {moved[label] / 1e6:8.1f} MB  "
                      f"{moved[label] / med / 1e3:6.0f} GB/s")
            del tr, src, dst, p_dst, params, stat, moments
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
