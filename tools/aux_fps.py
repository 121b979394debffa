#!/usr/bin/env python3
"""What the depth / alpha maps (GS_FRAME_AUX) cost on the headline scene (gs_scene CONFIGS["cfg5"]: 2.4 M Gaussians at
1920x1080):

  inference  frames/s with and without aux, culled (a camera at rest: GS_FRAME_OCCLUSION_CULL) and unculled;
  training   forward + backward steps/s with and without aux, rgb colours and SH degree 2.

Timing: warm-up steps first (clocks and caches to their steady state), then blocks of K steps with one frame in flight,
bracketed by torch.cuda.Event on the stream and a synchronize; the variants of a group are measured in ROUNDS interleaved
with each other (A/B/A/B on the same device, so that drift hits all alike) and the median block is reported with the
spread (min, max) of the blocks.  One JSON line per variant, then the aux / plain ratios.

    python tools/aux_fps.py [--steps 100] [--rounds 5] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_frame import FrameRenderer  # noqa: E402
from gs_scene import CONFIGS, make_camera, make_scene  # noqa: E402


def tensors(scene, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa,
                                                                       scene.rgb)]


def block_ms(step, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(k):
        step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / k


def measure(variants, steps, rounds, warmup):
    """variants: {name: step function} -> {name: [ms per step of every block]}, interleaved rounds."""
    for f in variants.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    out = {n: [] for n in variants}
    for _ in range(rounds):
        for n, f in variants.items():
            out[n].append(block_ms(f, steps))
    return out


def report(kind, res):
    rows = {}
    for n, ms in res.items():
        med = statistics.median(ms)
        rows[n] = med
        print(json.dumps({"kind": kind, "variant": n, "per_s": round(1000.0 / med, 1), "ms_median": round(med, 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "blocks": len(ms)}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, W, H, _ = CONFIGS["cfg5"]
    cam = make_camera(W, H)
    summary = {}

    # ---- inference: culled (camera at rest) / unculled, with and without the maps
    p = tensors(make_scene(n, W, H, seed=2023), dev)
    rend = {k: FrameRenderer(dev, max_pairs=1 << 23, auto_grow="async", occlusion_cull=(k[0] == "c"))
            for k in ("culled", "culled_aux", "unculled", "unculled_aux")}
    inf = {k: (lambda r=r, aux=k.endswith("aux"): r.forward(*p, cam, training=False, aux=aux)) for k, r in rend.items()}
    res = report("inference_fps", measure(inf, args.steps, args.rounds, args.warmup))
    for k in ("culled", "unculled"):
        assert (rend[k]._frame.flags & 256) == (256 if k == "culled" else 0)
        summary[f"inference_{k}_aux_cost"] = round(res[f"{k}_aux"] / res[k] - 1.0, 4)
    del rend, inf
    torch.cuda.empty_cache()

    # ---- training forward + backward (random dL/dimage, dL/ddepth, dL/dalpha), rgb and SH degree 2
    for label, use_sh in (("rgb", False), ("sh2", True)):
        q = tensors(make_scene(n, W, H, seed=2023, use_sh=use_sh, sh_degree=2), dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        gimg = torch.randn(H, W, 3, device=dev, generator=gen)
        gd = torch.randn(H, W, device=dev, generator=gen)
        ga = torch.randn(H, W, device=dev, generator=gen)
        rp = FrameRenderer(dev, max_pairs=1 << 23, training=True, auto_grow="async", bwd_rows=False)
        ra = FrameRenderer(dev, max_pairs=1 << 23, training=True, auto_grow="async", bwd_rows=False)
        outs = tuple(torch.empty_like(t) for t in q)

        def plain():
            rp.forward(*q, cam)
            rp.backward(gimg, out=outs)

        def aux():
            ra.forward(*q, cam, aux=True)
            ra.backward(gimg, out=outs, grad_depth=gd, grad_alpha=ga)

        res = report(f"training_{label}_it_s", measure({"plain": plain, "aux": aux}, max(args.steps // 4, 10), args.rounds,
                                                       args.warmup))
        summary[f"training_{label}_aux_cost"] = round(res["aux"] / res["plain"] - 1.0, 4)
        del rp, ra, q, outs
        torch.cuda.empty_cache()
    print(json.dumps({"kind": "summary", **summary}), flush=True)


if __name__ == "__main__":
    main()
