#!/usr/bin/env python3
"""What the per-view exposure costs, one MI355X:

  loss       gs_exposure_apply + gs_loss_track + gs_exposure_backward (sums and the device Adam step: gs_exposure.Exposure, free)
             against the gs_loss_track call they surround (gs_train.TrackLoss, with a range map, its finish kernel included), at
             160 x 120, 640 x 480 and 1920 x 1080;
  iteration  one gs_track.Tracker.iteration (forward, loss, pose backward, the read) with TrackOptions.fit_exposure against the
             same without, 160 x 120, a 20,000-Gaussian scene;
  track      a whole Tracker.track call (300 iterations) with and without the option, same scene.

Every leg in one process: blocks of calls between two device events, the two sides alternating block by block for `--rounds`
rounds after a warm-up block of each; per side the median of its blocks with the smallest and the largest block, per pair the
ratio of the medians and the spread the blocks of one side show among themselves (the protocol of tools/gate_map_cost.py).

    python tools/exposure_cost.py [--calls 200] [--rounds 7] [--out profiles/exposure.txt]

The report replaces the head of `--out`; whatever follows the line that starts with MARK (recorded test output) is kept.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))

SIZES = [("160x120", 120, 160), ("640x480", 480, 640), ("1920x1080", 1080, 1920)]
MARK = "---- recorded test output"


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
    """`sides`: {label: fn}, the first is the baseline.  Alternating blocks; -> the difference of the medians in us."""
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
    diff = statistics.median(n) - statistics.median(b)
    lines.append(json.dumps({"leg": name, "size": size, "what": f"{new} / {base}",
                             "ratio_of_medians": round(statistics.median(n) / statistics.median(b), 4),
                             "difference_us": round(diff, 2), "block_spread_us": round(spread, 2)}))
    return diff, statistics.median(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from gs_exposure import Exposure
    from gs_scene import make_camera, make_scene
    from gs_track import TrackOptions, Tracker
    from gs_train import TrackLoss

    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback"
    dev = torch.device("cuda:0")
    lines = []
    for size, H, W in SIZES:
        gen = torch.Generator(dev).manual_seed(H + W)
        x = torch.rand(H, W, 3, device=dev, generator=gen)
        y = (0.8 * x + 0.03 + 0.05 * torch.randn(H, W, 3, device=dev, generator=gen)).clamp(0, 1).contiguous()
        A = (0.02 + 0.98 * torch.rand(H, W, device=dev, generator=gen)).contiguous()
        z = (0.3 + 11.7 * torch.rand(H, W, device=dev, generator=gen)).contiguous()
        D = (A * z * (0.7 + 0.6 * torch.rand(H, W, device=dev, generator=gen))).contiguous()
        loss = TrackLoss(H, W, 0.5, 1.0 / 3.0, 1.0, 0.0, dev)
        ex = Exposure(H, W, dev)
        ex.free(3e-2, 3e-2)
        scale = 1.0 / (H * W)

        def plain():
            loss(x, D, A, y, z, scale)

        def compensated():
            gi, _, _ = loss(ex.apply(x), D, A, y, z, scale)
            ex.backward(x, gi)

        compare("loss", size, {"gs_loss_track": plain, "apply + gs_loss_track + backward (sums, Adam)": compensated},
                args.calls, args.rounds, lines)
    # a Tracker iteration and a whole call, 160 x 120
    H, W = 120, 160
    scene = make_scene(20_000, W, H, seed=103)
    cam = make_camera(W, H, yaw_deg=2.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
    off, on = Tracker(params, cam, TrackOptions(), dev), Tracker(params, cam, TrackOptions(fit_exposure=True), dev)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    img, _, d, a = off.renderer.forward(*params, cam, training=True, aux=True)
    target = (0.8 * img + 0.03).contiguous().clone()
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous().clone()
    next(iter(on._exposures.values())).free(3e-2, 3e-2)  # (the iteration steps the exposure, as inside track)
    diff, base = compare("iteration", "160x120", {"Tracker.iteration": lambda: off.iteration(R, t, target, rng),
                                                  "Tracker.iteration, fit_exposure": lambda: on.iteration(R, t, target, rng)},
                         args.calls, args.rounds, lines)
    lines.append(json.dumps({"leg": "iteration", "size": "160x120", "what": "share of an iteration",
                             "exposure_us_over_iteration_us": round(diff / base, 4), "above_a_tenth": bool(diff > 0.1 * base)}))
    compare("track", "160x120", {"Tracker.track (300 iterations)": lambda: off.track(target, rng, init=(R, t)),
                                 "Tracker.track, fit_exposure": lambda: on.track(target, rng, init=(R, t))},
            2, args.rounds, lines)
    head = ("Cost of the per-view exposure (tools/exposure_cost.py), one MI355X: device events around blocks of calls, the two sides "
            f"of a pair alternating for {args.rounds} rounds after a warm-up block each; us per call ({args.calls} calls per block; "
            "2 for a whole track call).")
    text = "\n".join([head] + lines) + "\n"
    print(text, end="")
    kept = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if MARK in old:
            kept = old[old.index(MARK):]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + kept)


if __name__ == "__main__":
    main()
