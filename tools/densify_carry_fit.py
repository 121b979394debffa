#!/usr/bin/env python3
"""What does carrying Adam's moments through densification (Trainer(densify_carry=True)) do to the fit?

    python tools/densify_carry_fit.py [--seeds 1,2,3,4,5] [--iters 7001] [--budget-s SECONDS]

The 7,001-iteration synthetic fit of tools/train_demo.py with the reference's densification schedule, once with the fresh Adam
behind every adaptive_control ("off", the default and the reference's behaviour) and once with the moments carried ("on"), for
several seeds (start perturbation, view order, split draws).  The method is tools/psnr_noise.py's: one fresh process per run,
the two arms alternate within a seed, same box.  Per run: held-out PSNR and SSIM, the final training loss, the final Gaussian
count, iterations per second; then mean / min / max per arm, and the off arm's own spread over the seeds -- the noise floor
any difference between the arms has to be read against.  Nothing here is a pass mark."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
a = sys.argv[1:]
seeds = [int(x) for x in (a[a.index("--seeds") + 1] if "--seeds" in a else "1,2,3,4,5").split(",")]
iters = a[a.index("--iters") + 1] if "--iters" in a else "7001"
budget = float(a[a.index("--budget-s") + 1]) if "--budget-s" in a else None  # start no seed that would not finish within it
ARMS = (("off", "--densify"), ("on", "--densify-carry"))
KEYS = ("test_psnr_after_dB", "test_ssim_after", "final_train_loss", "n_gaussians_end", "iters_per_s")
print(f"densify_carry fit: {iters} iterations, seeds {seeds}, arms off (fresh Adam behind every adaptive_control) / on (moments "
      "carried), one fresh process per run, off and on alternate within a seed", flush=True)
print(f"{'seed':>4} {'arm':>3} {'PSNR before':>11} {'PSNR dB':>8} {'SSIM':>7} {'final loss':>10} {'Gaussians':>10} {'it/s':>7}",
      flush=True)
rows, t_start, longest_seed = [], time.monotonic(), 0.0
for seed in seeds:
    if budget is not None and time.monotonic() - t_start + 1.2 * longest_seed > budget:
        print(f"--budget-s {budget:g}: seed {seed} and the seeds behind it are not started", flush=True)
        break
    t_seed = time.monotonic()
    for arm, flag in ARMS:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_demo.py"), iters, "--seed", str(seed), flag],
                           capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode or not line:
            print(f"{seed:>4} {arm:>3} FAILED (exit {p.returncode}): {p.stderr[-300:]!r}", flush=True)
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):  # the device may be gone: start nothing more on it
                sys.exit(1)
            continue
        d = json.loads(line[-1])
        d["arm"] = arm
        rows.append(d)
        print(f"{seed:>4} {arm:>3} {d['test_psnr_before_dB']:>11.2f} {d['test_psnr_after_dB']:>8.2f} {d['test_ssim_after']:>7.4f} "
              f"{d['final_train_loss']:>10.5f} {d['n_gaussians_end']:>10d} {d['iters_per_s']:>7.1f}", flush=True)
    longest_seed = max(longest_seed, time.monotonic() - t_seed)
print("per arm: mean (min .. max)")
stats = {}
for arm, _ in ARMS:
    mine = [r for r in rows if r["arm"] == arm]
    if not mine:
        continue
    stats[arm] = {}
    parts = [f"{arm:>3} ({len(mine)} runs)"]
    for k in KEYS:
        v = [float(r[k]) for r in mine]
        stats[arm][k] = (sum(v) / len(v), min(v), max(v))
        parts.append(f"{k} {stats[arm][k][0]:.5g} ({min(v):.5g} .. {max(v):.5g})")
    print("  " + "; ".join(parts))
if "off" in stats and "on" in stats:
    for k in KEYS[:3]:
        off, on = stats["off"][k], stats["on"][k]
        print(f"  {k}: on - off = {on[0] - off[0]:+.5g} (means); the off arm alone spans {off[2] - off[1]:.5g} over its seeds "
              "(the noise floor)")
    paired = [(r_on["test_psnr_after_dB"] - r_off["test_psnr_after_dB"])
              for r_off in rows if r_off["arm"] == "off"
              for r_on in rows if r_on["arm"] == "on" and r_on["seed"] == r_off["seed"]]
    if paired:
        print("  PSNR on - off per seed: " + ", ".join(f"{d:+.2f}" for d in paired))
