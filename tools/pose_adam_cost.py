#!/usr/bin/env python3
"""What the pose gradient costs inside a training step on the headline scene (gs_scene CONFIGS["cfg5"]: 2.4 M Gaussians at
1920x1080, rgb colours), in training steps per second of

  a  rgb_fused        the rgb-only step: forward, image loss kernel, backward with the Adam step fused in
  b  rgbd_fused       the RGB-D step of gs_train.Trainer: forward(aux=True), image loss, gs_loss_depth, backward_adam
  c  rgbd_pose_split  the RGB-D step with a pose gradient as it could be assembled before gs_frame_backward_adam_pose:
                      the same losses, backward(grad_pose=...) into gradient buffers, FusedAdam.step()
  d  rgbd_pose_fused  the step of a free view of gs_train.Trainer: backward_adam(grad_pose=...)

Timing as tools/rgbd_step_cost.py: warm-up steps, then blocks of K steps bracketed by events, the variants interleaved in
rounds on the same device; medians with the spread of the blocks.  d / c is what the fused pose step saves, d / b what the
pose gradient costs.  Kernel times (frame_project_backward_adam_pose_kernel against frame_project_backward_adam_aux_kernel,
pose_grad_finalize_kernel) come from the same script under the kernel tracer, in a run of its own:

    python tools/pose_adam_cost.py [--steps 50] [--rounds 5] [--warmup 15]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/pose_adam_cost.py --steps 20 --rounds 2
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
    fd, od, rd, ld = make()
    dl = DepthLoss(H, W, "residual", 0.5, dev)
    gp = (torch.zeros(3, 3, device=dev), torch.zeros(3, device=dev))

    def step_a():
        image, _ = ra.forward(*fa.params, cam)
        oa.skip_flag = ra.overflow_flag()
        ra.backward_adam(la(image, target), oa.fused_descriptor())

    def rgbd(r, flat, opt, loss):
        image, _, dm, am = r.forward(*flat.params, cam, aux=True)
        opt.skip_flag = r.overflow_flag()
        gimg = loss(image, target)
        gd, ga = dl(dm, am, zrange, weight / n_valid)
        return gimg, dict(grad_depth=gd, grad_alpha=ga)

    def step_b():
        gimg, maps = rgbd(rb, fb, ob, lb)
        rb.backward_adam(gimg, ob.fused_descriptor(), **maps)

    def step_c():
        gimg, maps = rgbd(rc, fc, oc, lc)
        rc.backward(gimg, out=fc.grads, grad_pose=gp, **maps)
        oc.step()

    def step_d():
        gimg, maps = rgbd(rd, fd, od, ld)
        rd.backward_adam(gimg, od.fused_descriptor(), grad_pose=gp, **maps)

    variants = {"a_rgb_fused": step_a, "b_rgbd_fused": step_b, "c_rgbd_pose_split": step_c, "d_rgbd_pose_fused": step_d}
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
    print(json.dumps({"summary": "step time ratios (medians)", "d_over_c": round(m["d_rgbd_pose_fused"] / m["c_rgbd_pose_split"], 4),
                      "d_over_b": round(m["d_rgbd_pose_fused"] / m["b_rgbd_fused"], 4),
                      "b_over_a": round(m["b_rgbd_fused"] / m["a_rgb_fused"], 4)}))


if __name__ == "__main__":
    main()
