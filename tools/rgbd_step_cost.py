#!/usr/bin/env python3
"""What depth supervision costs on the headline scene (gs_scene CONFIGS["cfg5"]: 2.4 M Gaussians at 1920x1080, rgb colours),
in training steps per second of

  a  rgb_fused       the rgb-only step: forward, image loss kernel, backward with the Adam step fused in
  b  rgbd_assembled  the RGB-D step a user could assemble before gs_loss_depth / gs_frame_backward_adam_aux existed:
                     forward(aux=True), image loss kernel, an L1 depth loss written in torch (autograd on the two maps),
                     backward(grad_depth, grad_alpha) into gradient buffers, FusedAdam.step()
  c  rgbd_fused      the RGB-D step of gs_train.Trainer: forward(aux=True), image loss kernel, gs_loss_depth,
                     backward_adam(grad_depth, grad_alpha)

Timing as tools/aux_fps.py: warm-up steps, then blocks of K steps bracketed by events, the variants interleaved in rounds on
the same device; medians with the spread of the blocks.  Requirement: c is not slower than b beyond that spread; c / a is the
cost of depth supervision.  Kernel times (gs_loss_depth, the aux variant of the fused projection backward against its twin)
come from the same script under the kernel tracer:

    python tools/rgbd_step_cost.py [--steps 50] [--rounds 5] [--warmup 15]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/rgbd_step_cost.py --steps 20 --rounds 2
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

from gs_dp import FlatGaussianParams  # noqa: E402
from gs_frame import FrameRenderer  # noqa: E402
from gs_scene import CONFIGS, make_camera, make_scene  # noqa: E402
from gs_train import DepthLoss, FusedAdam, ImageLoss, TrainOptions, base_lrs  # noqa: E402


def block_ms(step, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(k):
        step()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, W, H, _ = CONFIGS["cfg5"]
    scene = make_scene(n, W, H)
    cam = make_camera(W, H, yaw_deg=2.0)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa,
                                                                           scene.rgb)]
    # targets: the scene's own image and range map, slightly off, so that every step has a gradient
    r0 = FrameRenderer(dev, max_pairs=1 << 22, auto_grow=True)
    img, _, d, a = r0.forward(*params, cam, training=False, aux=True)
    target = (img * 0.9 + 0.05).clamp(0, 1).contiguous()
    zrange = torch.where(a >= 0.5, 1.02 * d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous()
    n_valid = int((zrange > 0).sum())
    weight = 0.2
    del r0
    lrs = [b * 1e-3 for b in base_lrs(TrainOptions())]  # tiny steps: the scene stays the scene that is measured

    def make():
        flat = FlatGaussianParams([t.clone() for t in params])
        opt = FusedAdam(flat, lrs, grad_stat="max")
        r = FrameRenderer(dev, max_pairs=1 << 22, training=True, auto_grow=True)
        return flat, opt, r, ImageLoss(H, W, 0.1, dev)

    fa, oa, ra, la = make()
    fb, ob, rb, lb = make()
    fc, oc, rc, lc = make()
    dl = DepthLoss(H, W, "residual", 0.5, dev)
    valid = zrange > 0

    def step_a():
        image, _ = ra.forward(*fa.params, cam)
        oa.skip_flag = ra.overflow_flag()
        ra.backward_adam(la(image, target), oa.fused_descriptor())

    def step_b():
        image, _, dm, am = rb.forward(*fb.params, cam, aux=True)
        ob.skip_flag = rb.overflow_flag()
        gimg = lb(image, target)
        dm_, am_ = dm.detach().requires_grad_(True), am.detach().requires_grad_(True)
        loss = (weight / n_valid) * torch.where(valid, dm_ - am_ * zrange, torch.zeros_like(dm_)).abs().sum()
        gd, ga = torch.autograd.grad(loss, (dm_, am_))
        rb.backward(gimg, out=fb.grads, grad_depth=gd, grad_alpha=ga)
        ob.step()

    def step_c():
        image, _, dm, am = rc.forward(*fc.params, cam, aux=True)
        oc.skip_flag = rc.overflow_flag()
        gimg = lc(image, target)
        gd, ga = dl(dm, am, zrange, weight / n_valid)
        rc.backward_adam(gimg, oc.fused_descriptor(), grad_depth=gd, grad_alpha=ga)

    variants = {"a_rgb_fused": step_a, "b_rgbd_assembled": step_b, "c_rgbd_fused": step_c}
    for f in variants.values():
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, f in variants.items():
            times[k].append(block_ms(f, args.steps))
    for k, v in times.items():
        med = statistics.median(v)
        print(json.dumps({"variant": k, "steps_per_s": round(1e3 / med, 1), "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "blocks": len(v), "steps_per_block": args.steps}))
    m = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"summary": "step time ratios (medians)", "c_over_b": round(m["c_rgbd_fused"] / m["b_rgbd_assembled"], 4),
                      "c_over_a": round(m["c_rgbd_fused"] / m["a_rgb_fused"], 4),
                      "b_over_a": round(m["b_rgbd_assembled"] / m["a_rgb_fused"], 4)}))


if __name__ == "__main__":
    main()
