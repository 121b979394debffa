#!/usr/bin/env python3
"""What the pose-only backward (gs_frame_backward_pose, TrackOptions.pose_only) saves in camera tracking, at 640x480 on the
376,467-Gaussian scene and at 1920x1080 on the 2.4 M scene (rgb colours), plain and aux (RGB-D) frames.

  kernels    under the kernel tracer, in a run of its own: per case and frame kind one forward and one raster backward, then
             blocks of K calls of backward(part=GS_BWD_GEOMETRY, grad_pose=...) -- frame_project_backward_pose_kernel<1> and,
             on aux frames, frame_aux_depth_pose_backward_kernel -- and of backward_pose(part=GS_BWD_GEOMETRY) --
             frame_pose_backward_kernel<AUX> --, interleaved in rounds, on the same gradient rows in the same process.  This leg
             prints the plan of its launches; `--summarise` turns the tracer's dispatch list into a time per kernel and block
             (the median of the block's dispatches), and reports per kernel the median over the blocks with their spread.
  iteration  tracer off: ms per Tracker.iteration over whole track() calls with TrackOptions.pose_only off and on, interleaved
             in rounds in one process; an iteration synchronises with the host, so the blocks are timed by the host clock
             around work that ends in a synchronise.  Medians with the spread of the blocks.

    python tools/pose_only_cost.py --leg iteration [--iters 60] [--rounds 5]
    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python tools/pose_only_cost.py --leg kernels [--calls 20] [--rounds 5]
    python tools/pose_only_cost.py --summarise OUT [--calls 20] [--rounds 5]        (no GPU; the same --calls / --rounds / --cases)

The rule for calling it faster (profiles/pose_only_cost.txt): the new kernel's median is below the sum of the medians of what it
replaces by more than the spread between blocks of the same variant, and the iteration is not slower beyond that spread.
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))

CASES = [("vga_376k", 376_467, 640, 480), ("1080p_2.4M", 2_400_000, 1920, 1080)]
KINDS = ("plain", "aux")
OLD_PROJ, OLD_AUX, NEW = "frame_project_backward_pose_kernel<1>", "frame_aux_depth_pose_backward_kernel", "frame_pose_backward_kernel"
WARMUP = 3  # calls of each side per (case, kind) in front of the blocks of the kernels leg


def selected(args):
    return [c for c in CASES if c[0] in args.cases.split(",")]


def scene_on_device(dev, n, W, H):
    import numpy as np
    import torch
    from gs_scene import make_camera, make_scene

    scene = make_scene(n, W, H)
    cam = make_camera(W, H, yaw_deg=2.0)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
    return params, cam


def kernels_leg(args):
    import torch
    from gaussian import _lib
    from gs_frame import FrameRenderer

    dev = torch.device("cuda:0")
    for name, n, W, H in selected(args):
        params, cam = scene_on_device(dev, n, W, H)
        for kind in KINDS:
            aux = kind == "aux"
            r = FrameRenderer(dev, max_pairs=1 << 22, training=True, occlusion_cull=False, auto_grow=True)
            r.forward(*params, cam, aux=aux)
            assert not r.last_frame_overflowed(wait=True)
            gen = torch.Generator(dev).manual_seed(5)
            gimg = torch.randn(H, W, 3, device=dev, generator=gen)
            maps = dict(grad_depth=torch.randn(H, W, device=dev, generator=gen) * 0.1,
                        grad_alpha=torch.randn(H, W, device=dev, generator=gen)) if aux else {}
            out = tuple(torch.empty_like(p) for p in params)
            r.backward(gimg, out=out, part=_lib.GS_BWD_RASTER, **maps)
            gp = (torch.zeros(3, 3, device=dev), torch.zeros(3, device=dev))
            gq = (torch.zeros(3, 3, device=dev), torch.zeros(3, device=dev))

            def old():
                r.backward(None, out=out, part=_lib.GS_BWD_GEOMETRY, grad_pose=gp)

            def new():
                r.backward_pose(None, gq, part=_lib.GS_BWD_GEOMETRY)

            for f in (old, new):
                for _ in range(WARMUP):
                    f()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for f in (old, new):
                    for _ in range(args.calls):
                        f()
                    torch.cuda.synchronize()
            same = bool(torch.equal(gp[0], gq[0]) and torch.equal(gp[1], gq[1]))
            print(json.dumps({"case": name, "kind": kind, "what": "kernels_plan", "warmup": WARMUP, "rounds": args.rounds,
                              "calls_per_block": args.calls, "pose_gradients_equal": same}), flush=True)
            del r
            torch.cuda.empty_cache()


def summarise(args):
    """The dispatches of the three kernels in start order; per (case, kind) each side has WARMUP + rounds x calls of them."""
    files = sorted(glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    seen = {OLD_PROJ: [], OLD_AUX: [], NEW: []}
    with open(files[0], newline="") as fh:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)))
    mangled = {OLD_PROJ: "frame_project_backward_pose_kernelILi1E", OLD_AUX: OLD_AUX, NEW: NEW}  # (a tracer that does not demangle)
    for t0, t1, k in rows:
        for key in seen:
            if key in k or mangled[key] in k:
                seen[key].append((t1 - t0) * 1e-3)
    per = WARMUP + args.rounds * args.calls
    pos = {k: 0 for k in seen}

    def blocks(key):
        v = seen[key][pos[key]:pos[key] + per]
        assert len(v) == per, (key, len(v), per)
        pos[key] += per
        return [statistics.median(v[WARMUP + b * args.calls:WARMUP + (b + 1) * args.calls]) for b in range(args.rounds)]

    for name, n, W, H in selected(args):
        for kind in KINDS:
            sides = {OLD_PROJ: blocks(OLD_PROJ), NEW: blocks(NEW)}
            if kind == "aux":
                sides[OLD_AUX] = blocks(OLD_AUX)
            for key, b in sides.items():
                print(json.dumps({"case": name, "kind": kind, "kernel": key, "us_median": round(statistics.median(b), 2),
                                  "us_block_min": round(min(b), 2), "us_block_max": round(max(b), 2), "blocks": len(b),
                                  "dispatches_per_block": args.calls}))
            old = [sum(x) for x in zip(*(b for key, b in sides.items() if key != NEW))]
            new = sides[NEW]
            spread = max(max(old) - min(old), max(new) - min(new))
            saved = statistics.median(old) - statistics.median(new)
            print(json.dumps({"case": name, "kind": kind, "what": "replaced_vs_new", "replaced_us_median": round(statistics.median(old), 2),
                              "new_us_median": round(statistics.median(new), 2), "saved_us": round(saved, 2),
                              "block_spread_us": round(spread, 2), "faster_beyond_spread": bool(saved > spread)}))
    assert all(pos[k] == len(seen[k]) for k in seen), ({k: len(v) for k, v in seen.items()}, pos)


def iteration_leg(args):
    import numpy as np
    import torch
    from gs_frame import FrameRenderer
    from gs_track import TrackOptions, Tracker, so3_exp

    dev = torch.device("cuda:0")
    for name, n, W, H in selected(args):
        params, cam = scene_on_device(dev, n, W, H)
        r = FrameRenderer(dev, max_pairs=1 << 22, training=False, occlusion_cull=False, auto_grow=True)
        img, _, d, a = r.forward(*params, cam, training=False, aux=True)
        tgt_rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous()
        tgt_img = img.contiguous().clone()
        del r
        R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
        R0 = so3_exp(np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98) * math.radians(0.5)) @ R_true
        t0 = t_true + np.array([0.6, 0.0, -0.8]) * 0.02
        for kind in KINDS:
            rng = tgt_rng if kind == "aux" else None
            trackers = {"pose_only_off": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=args.iters), dev),
                        "pose_only_on": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=args.iters, pose_only=True), dev)}
            res = {k: tr.track(tgt_img, rng, init=(R0, t0)) for k, tr in trackers.items()}  # (warm-up, and the same track?)
            same = bool(np.array_equal(res["pose_only_off"].rot, res["pose_only_on"].rot)
                        and res["pose_only_off"].losses == res["pose_only_on"].losses)
            times = {k: [] for k in trackers}
            for _ in range(args.rounds):
                for k, tr in trackers.items():
                    torch.cuda.synchronize()
                    t_ = time.perf_counter()
                    tr.track(tgt_img, rng, init=(R0, t0))
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t_) * 1e3 / args.iters)
            for k, v in times.items():
                print(json.dumps({"case": name, "kind": "rgbd" if kind == "aux" else "rgb", "what": "iteration", "side": k,
                                  "ms_median": round(statistics.median(v), 4), "ms_block_min": round(min(v), 4),
                                  "ms_block_max": round(max(v), 4), "blocks": len(v), "iterations_per_block": args.iters}), flush=True)
            off, on = times["pose_only_off"], times["pose_only_on"]
            spread = max(max(off) - min(off), max(on) - min(on))
            saved = statistics.median(off) - statistics.median(on)
            print(json.dumps({"case": name, "kind": "rgbd" if kind == "aux" else "rgb", "what": "iteration_off_vs_on",
                              "saved_ms": round(saved, 4), "block_spread_ms": round(spread, 4), "same_track": same,
                              "not_slower_beyond_spread": bool(saved > -spread), "faster_beyond_spread": bool(saved > spread)}),
                  flush=True)
            del trackers
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("kernels", "iteration"))
    ap.add_argument("--summarise", metavar="DIR", help="the tracer's output directory of a `--leg kernels` run")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    args = ap.parse_args()
    if args.summarise:
        summarise(args)
    elif args.leg == "kernels":
        kernels_leg(args)
    elif args.leg == "iteration":
        iteration_leg(args)
    else:
        ap.error("give --leg or --summarise")


if __name__ == "__main__":
    main()
