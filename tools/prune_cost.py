"""What a map edit costs: the prune kernel pair (gs_prune_classify + gs_prune_apply: three launches, timed with device
events, the counts taken from a call before: no host read), ``gs_prune.prune_rows`` with its host read of the counts and its
sixteen allocations, and the torch statement of the same edit (``mask = ...; [t[mask] for t in arrays]``: one mask, sixteen
boolean-mask gathers, each with its own host read of the count) -- all sixteen arrays of a carried prune (five parameter
arrays, ten moment arrays, the statistic), at 376 k and 2.4 M rows, rgb and SH degree 2 colours, with 1 %, 50 % and 99 % of
the rows removed.  The three are interleaved block by block; median over the blocks.

    python tools/prune_cost.py [--blocks 15] [--calls 20]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import torch  # noqa: E402

from gs_prune import opa_logit, prune_apply, prune_classify, prune_options, prune_rows  # noqa: E402

OPA_MIN = 0.005


def make_arrays(n, color_dim, removed_share, dev, seed):
    """pos, quat, scale, opa, rgb, their ten moment arrays and a statistic: 16 arrays; ``removed_share`` of the opacity logits
    lie below the threshold, at random rows."""
    g = torch.Generator(device=dev).manual_seed(seed)
    widths = (3, 4, 3, 1, color_dim)
    params = [torch.randn((n, w) if w > 1 else (n,), device=dev, generator=g) for w in widths]
    params[2] = params[2].abs() * 0.02
    gone = torch.rand(n, device=dev, generator=g) < removed_share
    t = opa_logit(OPA_MIN)
    params[3] = torch.where(gone, torch.full_like(params[3], t - 2.0), params[3].abs() + (t + 1.0))
    arrays = list(params)
    for p in params:
        arrays += [torch.randn_like(p), torch.rand_like(p)]
    arrays.append(torch.rand((n, 3), device=dev, generator=g))
    return arrays


def block_time(fn, calls):
    tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tic.record()
    for _ in range(calls):
        fn()
    toc.record()
    toc.synchronize()
    return tic.elapsed_time(toc) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    print(f"prune of 16 arrays: microseconds per call, median (min .. max) over {a.blocks} interleaved blocks of {a.calls} calls")
    worst = math.inf
    for n in (376_000, 2_400_000):
        for color_dim, cname in ((3, "rgb"), (27, "SH degree 2")):
            for share in (0.01, 0.5, 0.99):
                arrays = make_arrays(n, color_dim, share, dev, seed=n % 1000 + color_dim)
                scale, opa = arrays[2], arrays[3]
                opts = prune_options(OPA_MIN, None, "abs")
                thresh = opa_logit(OPA_MIN)
                counts, ws = prune_classify(scale, opa, opts)
                kept, removed = counts.tolist()
                dst = [torch.empty((kept,) + tuple(t.shape[1:]), device=dev) for t in arrays]

                def kernels():
                    c, w = prune_classify(scale, opa, opts)
                    prune_apply(arrays, dst, n, c, w)

                def with_read():
                    return prune_rows(scale, opa, arrays, opa_min=OPA_MIN, scale_max=None, scale_activation="abs")

                def torch_statement():
                    mask = (opa > thresh) & (scale.abs().square().sum(-1).sqrt() < math.inf)
                    return [t[mask] for t in arrays]

                got, ref = with_read()[0], torch_statement()
                assert all(torch.equal(x, y) for x, y in zip(got, ref)), "prune_rows and the torch statement disagree"
                row_bytes = 4 * sum(int(math.prod(t.shape[1:])) for t in arrays)
                fns = (("kernel pair (3 launches)", kernels), ("prune_rows (+ host read)", with_read),
                       ("torch: mask + 16 gathers", torch_statement))
                for _, fn in fns:  # warm-up: every shape the timed window uses
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                times = {label: [] for label, _ in fns}
                for _ in range(a.blocks):
                    for label, fn in fns:
                        times[label].append(block_time(fn, a.calls))
                med = {label: statistics.median(v) for label, v in times.items()}
                moved = kept * row_bytes * 2 + n * 16  # rows read and written + the decision's 16 bytes per row
                print(f"{n} rows, {cname} ({row_bytes} B per row), {removed} removed ({100.0 * removed / n:.1f} %):")
                for label, _ in fns:
                    v = times[label]
                    print(f"    {label:28s} {med[label]:10.1f} ({min(v):.1f} .. {max(v):.1f})")
                ratio = med["torch: mask + 16 gathers"] / med["prune_rows (+ host read)"]
                worst = min(worst, ratio)
                print(f"    torch / prune_rows {ratio:.2f}x; torch / kernel pair "
                      f"{med['torch: mask + 16 gathers'] / med['kernel pair (3 launches)']:.2f}x; the kernel pair moves "
                      f"{moved / 1e6:.1f} MB: {moved / med['kernel pair (3 launches)'] / 1e3:.0f} GB/s")
                del arrays, dst, got, ref
                torch.cuda.empty_cache()
    print(f"smallest torch / prune_rows ratio over all cases: {worst:.2f}x")


if __name__ == "__main__":
    main()
