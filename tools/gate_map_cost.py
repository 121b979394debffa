#!/usr/bin/env python3
"""What carrying the tracker's gate into mapping costs per call, at 640 x 480 and 1920 x 1080, one MI355X:

  loss   gs_loss_l1_ssim_weighted (gs_train.WeightedImageLoss, an all-ones map: the work does not depend on the weights) against
         gs_loss_l1_ssim (gs_train.ImageLoss), ssim_weight 0.1, each call with its finish kernel;
  mask   one gs_track_gate_mask call (gs_train.GateMask: memset, residual pass, two digit passes, mask pass, count sum) against
         one gs_loss_track_gated call (gs_train.GatedTrackLoss: the same with the loss pass and its sum), k_d = 10.

Both legs in one process: blocks of `--calls` calls between two device events, the two sides alternating block by block for
`--rounds` rounds after a warm-up block of each; per side the median of its blocks with the smallest and the largest block,
and per pair the ratio of the medians with the spread that the blocks of one side show among themselves.  With an all-ones map
the two losses' gradients are compared bit for bit in passing.

    python tools/gate_map_cost.py [--calls 200] [--rounds 7] [--out profiles/gate_map.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))

SIZES = [("640x480", 480, 640), ("1920x1080", 1080, 1920)]


def block_us(fn, calls):
    """us per call of `calls` calls of fn between two device events."""
    import torch

    tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tic.record()
    for _ in range(calls):
        fn()
    toc.record()
    toc.synchronize()
    return tic.elapsed_time(toc) * 1e3 / calls


def compare(name, size, sides, calls, rounds, lines):
    """`sides`: {label: fn}, the first is the baseline.  Alternating blocks; -> the report lines."""
    for fn in sides.values():
        block_us(fn, calls)  # warm-up: code objects, caches
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(block_us(fn, calls))
    for k, v in times.items():
        lines.append(json.dumps({"leg": name, "size": size, "side": k, "us_median": round(statistics.median(v), 2),
                                 "us_block_min": round(min(v), 2), "us_block_max": round(max(v), 2), "blocks": len(v),
                                 "calls_per_block": calls}))
    (base, b), (new, n) = times.items()
    spread = max(max(b) - min(b), max(n) - min(n))
    lines.append(json.dumps({"leg": name, "size": size, "what": f"{new} / {base}",
                             "ratio_of_medians": round(statistics.median(n) / statistics.median(b), 4),
                             "difference_us": round(statistics.median(n) - statistics.median(b), 2),
                             "block_spread_us": round(spread, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_map.txt"))
    args = ap.parse_args()

    import torch
    from gs_train import GatedTrackLoss, GateMask, ImageLoss, WeightedImageLoss, weight_sums

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback"
    dev = torch.device("cuda:0")
    lines = []
    for size, H, W in SIZES:
        gen = torch.Generator(dev).manual_seed(H + W)
        x = torch.rand(H, W, 3, device=dev, generator=gen)
        y = (x + 0.1 * torch.randn(H, W, 3, device=dev, generator=gen)).clamp(0, 1).contiguous()
        ones = torch.ones(H, W, device=dev)
        sums = weight_sums(ones)
        plain, weighted = ImageLoss(H, W, 0.1, dev), WeightedImageLoss(H, W, 0.1, dev)
        compare("loss", size, {"gs_loss_l1_ssim": lambda: plain(x, y),
                               "gs_loss_l1_ssim_weighted": lambda: weighted(x, y, ones, *sums)}, args.calls, args.rounds, lines)
        same = bool(torch.equal(plain.grad, weighted.grad) and torch.equal(plain.values, weighted.values))
        lines.append(json.dumps({"leg": "loss", "size": size, "what": "all-ones weights", "bitwise_equal_to_unweighted": same}))
        # a frame of the map and an incoming frame: alpha straddles alpha_min, the expected depth is within 30 % of the range
        A = (0.02 + 0.98 * torch.rand(H, W, device=dev, generator=gen)).contiguous()
        z = (0.3 + 11.7 * torch.rand(H, W, device=dev, generator=gen)).contiguous()
        D = (A * z * (0.7 + 0.6 * torch.rand(H, W, device=dev, generator=gen))).contiguous()
        gated = GatedTrackLoss(H, W, 0.5, 1.0 / 3.0, 1.0, 10.0, 0.0, 0.0, 0.0, True, dev)
        mask = GateMask(H, W, 0.5, 10.0, 0.0, 0.0, 0.0, True, dev)
        scale = 1.0 / (H * W)
        compare("mask", size, {"gs_loss_track_gated": lambda: gated(x, D, A, y, z, scale),
                               "gs_track_gate_mask": lambda: mask(x, D, A, y, z)}, args.calls, args.rounds, lines)
        lines.append(json.dumps({"leg": "mask", "size": size, "what": "same medians",
                                 "equal": bool(torch.equal(gated.values[5:8], mask.values[5:8]))}))
    head = ("Per-call cost of the gate carried into mapping (tools/gate_map_cost.py), one MI355X: device events around blocks of "
            f"{args.calls} calls, the two sides of a pair alternating for {args.rounds} rounds after a warm-up block each; us per call.")
    text = "\n".join([head] + lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
