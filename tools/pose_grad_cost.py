#!/usr/bin/env python3
"""What the camera pose gradient (GS_FRAME_POSE_GRAD) costs on the headline scene (gs_scene CONFIGS["cfg5"]: 2.4 M Gaussians
at 1920x1080, rgb colours): training forward + backward steps with and without the flag, alternated in the same process,
with and without the depth / alpha maps.

Meant to run under the kernel tracer, which gives the per-kernel times (the pose variant of the projection backward against
the plain one, the finalize kernel):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/pose_grad_cost.py [--steps 50]

It also prints, per variant, the median ms per step over interleaved blocks (torch.cuda.Event), as tools/aux_fps.py does.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, W, H, _ = CONFIGS["cfg5"]
    scene = make_scene(n, W, H)
    cam = make_camera(W, H, yaw_deg=2.0)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa,
                                                                           scene.rgb)]
    r = FrameRenderer(dev, max_pairs=1 << 22, training=True, auto_grow=True)
    gimg = torch.randn(H, W, 3, device=dev) * 1e-3
    gmap = torch.randn(H, W, device=dev) * 1e-3
    grads = tuple(torch.empty_like(p) for p in params)
    gp = (torch.empty(3, 3, device=dev), torch.empty(3, device=dev))

    def step(aux, pose):
        r.forward(*params, cam, aux=aux)
        kw = dict(grad_depth=gmap, grad_alpha=gmap) if aux else {}
        r.backward(gimg, out=grads, grad_pose=gp if pose else None, **kw)

    variants = {f"{'aux_' if aux else ''}{'pose' if pose else 'plain'}": (aux, pose)
                for aux in (False, True) for pose in (False, True)}
    for aux, pose in variants.values():
        for _ in range(args.warmup):
            step(aux, pose)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (aux, pose) in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(args.steps):
                step(aux, pose)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / args.steps)
    for k, v in times.items():
        print(json.dumps({"variant": k, "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "blocks": len(v)}))
    m = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"summary": "pose / plain step time", "rgb": round(m["pose"] / m["plain"], 4),
                      "rgb_aux": round(m["aux_pose"] / m["aux_plain"], 4)}))


if __name__ == "__main__":
    main()
