#!/usr/bin/env python3
"""What camera tracking costs (gs_loss_track, gs_track.Tracker), at 640x480 on the 376,467-Gaussian scene and at 1920x1080 on
the 2.4 M scene (rgb colours), each against what the tree offered before:

  loss       us per call of the kernel pair (track_loss_kernel + finalize, through gs_train.TrackLoss) against the torch
             restatement of the same loss -- masks, |I - T|, |D / A - z|, the sum, and autograd for the three gradient maps;
  iteration  ms per tracking iteration of Tracker.track (forward, loss kernel, RASTER + GEOMETRY backward with the pose
             gradient, one 64-byte read, the host SE(3) step) against the same iteration assembled as
             tests/test_gpu_pose.py::test_pose_recovery(with_depth=True) does it: autograd render_aux(pose=...), a masked
             torch loss, loss.backward() (the whole backward), torch.optim.Adam on (w, tran).

  gate       the median gate (gs_loss_track_gated, TrackOptions.depth_gate_k = 10): us per call of its kernel chain (one
             memset, residual pass, two digit passes, gated loss pass, finalize; through gs_train.GatedTrackLoss) against
             the ungated pair, and ms per Tracker iteration with the gate on against the gate off -- the ungated side is the
             code of the legs above, unchanged by the gate, and is the baseline.

  pyramid    coarse to fine (gs_pyramid_down, TrackOptions.pyramid): us per gs_pyramid_down beside the bytes it moves; ms per
             Tracker iteration at pyramid levels 0 / 1 / 2; ms per track() under the schedule ((2, 100), (1, 100), (0, 100))
             against 300 level-0 iterations, interleaved in one process; and -- once, whatever --cases says -- on the
             160 x 120 scene of tests/test_gpu_track.py the final pose errors from starts 0.5 deg / 0.02, 1 / 0.04, 2 / 0.08
             and 4 / 0.16 off, with and without the schedule.

Protocol of tools/rgbd_step_cost.py: warm-up, then blocks of K calls, the two sides interleaved in rounds in one process;
medians with the spread of the blocks.  The loss blocks are bracketed by device events; an iteration synchronises with the
host on both sides, so those blocks are timed by the host clock around work that ends in a synchronise.

    python tools/track_cost.py [--calls 200] [--iters 60] [--rounds 5] [--legs loss,iteration,gate,pyramid]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_frame import FrameRenderer  # noqa: E402
from gs_scene import make_camera, make_scene  # noqa: E402
from gs_track import TrackOptions, Tracker, so3_exp  # noqa: E402
from gs_train import GatedTrackLoss, TrackLoss  # noqa: E402

CASES = [("vga_376k", 376_467, 640, 480), ("1080p_2.4M", 2_400_000, 1920, 1080)]


def events_us(fn, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(k):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / k


def axis_angle(w):
    K = torch.zeros(3, 3, dtype=w.dtype)
    K[0, 1], K[0, 2], K[1, 2] = -w[2], w[1], -w[0]
    K[1, 0], K[2, 0], K[2, 1] = w[2], -w[1], w[0]
    return torch.linalg.matrix_exp(K)


def report(case, what, unit, times):
    for k, v in times.items():
        print(json.dumps({"case": case, "what": what, "variant": k, f"{unit}_median": round(statistics.median(v), 3),
                          f"{unit}_min": round(min(v), 3), f"{unit}_max": round(max(v), 3), "blocks": len(v)}), flush=True)
    a, b = (statistics.median(times[k]) for k in ("fused", "assembled"))
    sa, sb = (max(times[k]) - min(times[k]) for k in ("fused", "assembled"))
    print(json.dumps({"case": case, "what": what, "fused_over_assembled": round(a / b, 4),
                      "faster_beyond_the_spread": bool(max(times["fused"]) < min(times["assembled"])),
                      "spread_fused": round(sa, 3), "spread_assembled": round(sb, 3)}), flush=True)


def report_gate(case, what, unit, times):
    for k, v in times.items():
        print(json.dumps({"case": case, "what": what, "variant": k, f"{unit}_median": round(statistics.median(v), 3),
                          f"{unit}_min": round(min(v), 3), f"{unit}_max": round(max(v), 3), "blocks": len(v)}), flush=True)
    a, b = (statistics.median(times[k]) for k in ("gated", "ungated"))
    print(json.dumps({"case": case, "what": what, "gated_over_ungated": round(a / b, 4),
                      f"gated_minus_ungated_{unit}": round(a - b, 3),
                      "spread_gated": round(max(times["gated"]) - min(times["gated"]), 3),
                      "spread_ungated": round(max(times["ungated"]) - min(times["ungated"]), 3)}), flush=True)


def gate_leg(args, name, dev, params, cam, maps, targets, start, H, W):
    """Gate off and on, interleaved: the kernel chain on the maps of the frame rendered from the start pose, then Tracker
    iterations.  k = 10 (SplaTAM's factor), coupled: the options of tests/test_gpu_track_gate.py."""
    img, d, a = maps
    tgt_img, tgt_rng = targets
    R0, t0 = start
    o = TrackOptions()
    scale = 1.0 / (H * W)
    tl = TrackLoss(H, W, o.alpha_min, o.color_weight, o.depth_weight, 0.0, dev)
    gl = GatedTrackLoss(H, W, o.alpha_min, o.color_weight, o.depth_weight, 10.0, 0.0, 0.0, 0.0, True, dev)
    sides = {"ungated": lambda: tl(img, d, a, tgt_img, tgt_rng, scale), "gated": lambda: gl(img, d, a, tgt_img, tgt_rng, scale)}
    for f in sides.values():
        for _ in range(args.warmup):
            f()
    v = gl.values.cpu().numpy()
    print(json.dumps({"case": name, "what": "gate_frame", "n_d": int(v[7]), "depth_counted": int(v[3]),
                      "colour_counted": int(v[4]), "m_d": float(v[5]), "m_c": float(v[6])}), flush=True)
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, f in sides.items():
            times[k].append(events_us(f, args.calls))
    report_gate(name, "gate_loss", "us", times)
    trackers = {"ungated": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=args.iters), dev),
                "gated": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=args.iters, depth_gate_k=10.0), dev)}
    for tr in trackers.values():
        tr.track(tgt_img, tgt_rng, init=(R0, t0))
    times = {k: [] for k in trackers}
    for _ in range(args.rounds):
        for k, tr in trackers.items():
            torch.cuda.synchronize()
            t_ = time.perf_counter()
            tr.track(tgt_img, tgt_rng, init=(R0, t0))
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t_) * 1e3 / args.iters)
    report_gate(name, "gate_iteration", "ms", times)


PYRAMID_SCHEDULE = ((2, 100), (1, 100), (0, 100))


def report_sides(case, what, unit, times, extra=None):
    for k, v in times.items():
        row = {"case": case, "what": what, "variant": k, f"{unit}_median": round(statistics.median(v), 3),
               f"{unit}_min": round(min(v), 3), f"{unit}_max": round(max(v), 3), "blocks": len(v)}
        row.update((extra or {}).get(k, {}))
        print(json.dumps(row), flush=True)


def pyramid_leg(args, name, dev, params, cam, targets, start, H, W):
    """gs_pyramid_down alone (device events), one Tracker iteration per level and a whole track() with and without the
    schedule (host clock around work that ends in a synchronise), the sides interleaved in rounds."""
    from gs_pyramid import Pyramid

    tgt_img, tgt_rng = targets
    R0, t0 = start
    pyr = Pyramid(H, W, 2, dev)
    one = Pyramid(H, W, 1, dev)
    images, ranges = pyr.build(tgt_img, tgt_rng)
    rgb = Pyramid(H, W, 1, dev)
    sides = {"rgbd": lambda: one.build(tgt_img, tgt_rng), "rgb_only": lambda: rgb.build(tgt_img)}
    for f in sides.values():
        for _ in range(args.warmup):
            f()
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, f in sides.items():
            times[k].append(events_us(f, args.calls))
    report_sides(name, "pyramid_down", "us", times,  # 16 bytes in and 4 out per fine pixel; RGB only 12 and 3
                 {"rgbd": {"bytes": H * W * 20}, "rgb_only": {"bytes": H * W * 15}})
    tr = Tracker(params, cam, TrackOptions(max_pairs=1 << 22, pyramid=((2, 1), (1, 1), (0, 1))), dev)
    its = {f"level{l}": (lambda l=l: tr.iteration(R0, t0, images[l], ranges[l], level=l)) for l in (0, 1, 2)}
    for f in its.values():
        for _ in range(args.warmup):
            f()
    times = {k: [] for k in its}
    for _ in range(args.rounds):
        for k, f in its.items():
            torch.cuda.synchronize()
            t_ = time.perf_counter()
            for _ in range(args.iters):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t_) * 1e3 / args.iters)
    report_sides(name, "pyramid_iteration", "ms", times)
    del tr
    trackers = {"schedule": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, pyramid=PYRAMID_SCHEDULE), dev),
                "level0_x300": Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=300), dev)}
    for tr in trackers.values():
        tr.track(tgt_img, tgt_rng, init=(R0, t0))
    times = {k: [] for k in trackers}
    for _ in range(args.rounds):
        for k, tr in trackers.items():
            torch.cuda.synchronize()
            t_ = time.perf_counter()
            tr.track(tgt_img, tgt_rng, init=(R0, t0))
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t_) * 1e3)
    report_sides(name, "pyramid_track", "ms", times)
    a, b = (statistics.median(times[k]) for k in ("schedule", "level0_x300"))
    print(json.dumps({"case": name, "what": "pyramid_track", "schedule": list(PYRAMID_SCHEDULE),
                      "schedule_over_level0_x300": round(a / b, 4)}), flush=True)


def pyramid_basin(dev):
    """The 160 x 120 scene of tests/test_gpu_track.py (make_scene(20,000, seed 103), yaw 2 degrees, tran (0.03, -0.01, 0.2)),
    targets rendered from the true pose, with depth: final pose errors from four starts, with and without the schedule."""
    W, H = 160, 120
    scene = make_scene(20_000, W, H, seed=103)
    cam = make_camera(W, H, yaw_deg=2.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa,
                                                                           scene.rgb)]
    r = FrameRenderer(dev, max_pairs=1 << 19, training=False, occlusion_cull=False, auto_grow=True)
    img, _, d, a = r.forward(*params, cam, training=False, aux=True)
    rng_map = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous()
    img = img.contiguous()
    R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
    trackers = {"schedule": Tracker(params, cam, TrackOptions(pyramid=PYRAMID_SCHEDULE), dev),
                "level0_x300": Tracker(params, cam, TrackOptions(), dev)}
    g = np.random.default_rng(107)  # (the draws of tests/track_ref.py::perturbed_start)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    sh = g.normal(size=3)
    sh /= np.linalg.norm(sh)
    for deg, shift in ((0.5, 0.02), (1.0, 0.04), (2.0, 0.08), (4.0, 0.16)):
        R0, t0 = so3_exp(axis * math.radians(deg)) @ R_true, t_true + sh * shift
        for k, tr in trackers.items():
            for depth in (True, False):
                tr.reset()
                res = tr.track(img, rng_map if depth else None, init=(R0, t0))
                e_r = float(np.linalg.norm(res.rot - R_true) / math.sqrt(2.0))
                e_t = float(np.linalg.norm(res.tran - t_true))
                print(json.dumps({"case": "test_scene_160x120", "what": "pyramid_basin", "variant": k, "with_depth": depth,
                                  "start_deg": deg, "start_shift": shift, "start_rot_err": round(math.radians(deg), 6),
                                  "rot_err": float(f"{e_r:.3e}"), "tran_err": float(f"{e_t:.3e}"),
                                  "to_a_tenth": bool(e_r <= 0.1 * math.radians(deg) and e_t <= 0.1 * shift),
                                  "loss": float(f"{res.loss:.4e}")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--legs", default="loss,iteration,gate")
    args = ap.parse_args()
    legs = args.legs.split(",")
    dev = torch.device("cuda:0")
    if "pyramid" in legs:
        pyramid_basin(dev)
    for name, n, W, H in CASES:
        if name not in args.cases.split(","):
            continue
        scene = make_scene(n, W, H)
        cam = make_camera(W, H, yaw_deg=2.0)
        params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa,
                                                                               scene.rgb)]
        r = FrameRenderer(dev, max_pairs=1 << 22, training=True, occlusion_cull=False, auto_grow=True)
        with torch.no_grad():
            tgt_img, tgt_d, tgt_a = r.render_aux(*params, cam)
        tgt_rng = torch.where(tgt_a > 0.5, tgt_d / tgt_a.clamp_min(1e-3), torch.zeros_like(tgt_d)).contiguous()
        tgt_img = tgt_img.contiguous()
        R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
        R0 = so3_exp(np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98) * math.radians(0.5)) @ R_true
        t0 = t_true + np.array([0.6, 0.0, -0.8]) * 0.02
        o = TrackOptions(max_pairs=1 << 22)
        scale = 1.0 / (H * W)

        # ---- the loss alone, on the maps of the frame rendered from the start pose
        c0 = make_camera(W, H)
        c0.rot, c0.tran = R0.astype(np.float32), t0.astype(np.float32)
        img, _, d, a = r.forward(*params, c0, training=True, aux=True)
        tl = TrackLoss(H, W, o.alpha_min, o.color_weight, o.depth_weight, o.depth_gate, dev)
        measured = tgt_rng > 0

        def loss_fused():
            tl(img, d, a, tgt_img, tgt_rng, scale)

        def loss_torch():
            i_, d_, a_ = (x.detach().requires_grad_(True) for x in (img, d, a))
            inside = a_.detach() >= o.alpha_min
            colour = ((i_ - tgt_img).abs().sum(-1) * inside).sum() * (scale * o.color_weight)
            depth = ((d_ / a_.clamp_min(1e-6) - tgt_rng).abs() * (inside & measured)).sum() * (scale * o.depth_weight)
            return torch.autograd.grad(colour + depth, (i_, d_, a_))

        if "gate" in legs:
            gate_leg(args, name, dev, params, cam, (img, d, a), (tgt_img, tgt_rng), (R0, t0), H, W)
        if "pyramid" in legs:
            pyramid_leg(args, name, dev, params, cam, (tgt_img, tgt_rng), (R0, t0), H, W)
        if "loss" not in legs and "iteration" not in legs:
            del r, params, tl
            torch.cuda.empty_cache()
            continue

        got, want = tl(img, d, a, tgt_img, tgt_rng, scale), loss_torch()
        for g, w_ in zip(got, want):  # the two sides state the same loss
            assert float((g - w_).abs().max()) <= 1e-5 * float(w_.abs().max()), "the torch restatement disagrees"
        sides = {"fused": loss_fused, "assembled": loss_torch}
        for f in sides.values():
            for _ in range(args.warmup):
                f()
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, f in sides.items():
                times[k].append(events_us(f, args.calls))
        report(name, "loss", "us", times)

        # ---- one tracking iteration
        tr = Tracker(params, cam, TrackOptions(max_pairs=1 << 22, iterations=args.iters), dev)

        def iters_fused():
            tr.track(tgt_img, tgt_rng, init=(R0, t0))

        R0t, t0t = torch.from_numpy(R0), torch.from_numpy(t0)

        def iters_assembled():
            w = torch.zeros(3, dtype=torch.float64, requires_grad=True)
            t = t0t.clone().requires_grad_(True)
            opt = torch.optim.Adam([w, t], lr=2e-3)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.01 ** (k / args.iters))
            for _ in range(args.iters):
                opt.zero_grad()
                rot = (axis_angle(w) @ R0t).float()
                im, dd, aa = r.render_aux(*params, cam, pose=(rot, t.float()))
                ed = dd / aa.clamp_min(1e-3)
                mask = (tgt_a > 0.5) & (aa.detach() > 0.5)
                loss = (im - tgt_img).abs().mean() + ((ed - tgt_rng).abs() * mask).mean()
                loss.backward()
                opt.step()
                sched.step()

        sides = {"fused": iters_fused, "assembled": iters_assembled}
        for f in sides.values():
            f()
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, f in sides.items():
                torch.cuda.synchronize()
                t_ = time.perf_counter()
                f()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t_) * 1e3 / args.iters)
        report(name, "iteration", "ms", times)
        del tr, r, params, tl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
