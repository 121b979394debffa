#!/usr/bin/env python3
"""What the device-resident pose (TrackOptions.device_pose: GS_FRAME_DEVICE_POSE frames + gs_pose_step) does to the wall time
of Tracker.track, with the default options (300 iterations) and a range map, at two sizes: the 20,000-Gaussian scene at
160 x 120 (tests/test_gpu_track.py's) and the 376,467-Gaussian scene of bench.py's cfg2 at 640 x 480.

Three legs -- the default tracker, pose_only=True and device_pose=True -- timed in interleaved blocks in ONE process, tracer
off: a block is one track() call between two device synchronisations, by the host clock.  Per leg the median over the blocks
and their spread (min, max); per size the verdict of profiles/track_device_cost.txt: the device-pose leg is not slower than
the pose_only leg by more than the spread of the blocks.  The three legs start from the same pose; the first two return the
same track bit for bit (tests/test_gpu_pose_only.py), the third the same to the rounding of its step (its frames are the host
path's frames at its logged poses: tests/test_gpu_device_pose.py) -- the pose errors are printed beside the times.

    python tools/track_device_cost.py [--rounds 7] [--iters 300] [--cases small_20k,vga_376k]
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

CASES = [("small_20k", 20_000, 160, 120, 103, 1 << 20), ("vga_376k", 376_467, 640, 480, 2023, 1 << 22)]
LEGS = [("default", {}), ("pose_only", {"pose_only": True}), ("device_pose", {"device_pose": True})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    args = ap.parse_args()
    import numpy as np
    import torch
    from gs_frame import FrameRenderer
    from gs_scene import make_camera, make_scene
    from gs_track import TrackOptions, Tracker, so3_exp

    dev = torch.device("cuda:0")
    for name, n, W, H, seed, max_pairs in CASES:
        if name not in args.cases.split(","):
            continue
        scene, cam = make_scene(n, W, H, seed=seed), make_camera(W, H, yaw_deg=2.0)
        cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
        params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
        r = FrameRenderer(dev, max_pairs=max_pairs, training=False, occlusion_cull=False, auto_grow=True)
        img, _, d, a = r.forward(*params, cam, training=False, aux=True)
        tgt_rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous()
        tgt_img = img.contiguous().clone()
        del r
        R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
        R0 = so3_exp(np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98) * math.radians(0.5)) @ R_true
        t0 = t_true + np.array([0.6, 0.0, -0.8]) * 0.02
        trackers = {leg: Tracker(params, cam, TrackOptions(max_pairs=max_pairs, iterations=args.iters, **kw), dev) for leg, kw in LEGS}
        res = {leg: tr.track(tgt_img, tgt_rng, init=(R0, t0)) for leg, tr in trackers.items()}  # (warm-up, and the tracks)
        times = {leg: [] for leg in trackers}
        for _ in range(args.rounds):
            for leg, tr in trackers.items():
                torch.cuda.synchronize()
                t_ = time.perf_counter()
                tr.track(tgt_img, tgt_rng, init=(R0, t0))
                torch.cuda.synchronize()
                times[leg].append((time.perf_counter() - t_) * 1e3)
        for leg, v in times.items():
            rr = res[leg]
            # (|R R_true^T - I|_F / sqrt 2 = 2 sin(angle / 2): exact for small angles, where arccos of the trace returns 0)
            ang = float(np.linalg.norm(rr.rot @ R_true.T - np.eye(3)) / math.sqrt(2.0))
            print(json.dumps({"case": name, "gaussians": n, "size": [W, H], "leg": leg, "iterations": args.iters,
                              "track_ms_median": round(statistics.median(v), 3), "track_ms_block_min": round(min(v), 3),
                              "track_ms_block_max": round(max(v), 3), "blocks": len(v),
                              "ms_per_iteration": round(statistics.median(v) / args.iters, 4), "attempts": rr.attempts,
                              "loss": rr.loss, "rot_err_rad": ang, "tran_err": float(np.linalg.norm(rr.tran - t_true))}), flush=True)
        same = bool(np.array_equal(res["default"].rot, res["pose_only"].rot) and res["default"].losses == res["pose_only"].losses)
        po, dp = times["pose_only"], times["device_pose"]
        spread = max(max(po) - min(po), max(dp) - min(dp))
        saved = statistics.median(po) - statistics.median(dp)
        print(json.dumps({"case": name, "what": "pose_only_vs_device_pose", "saved_ms": round(saved, 3),
                          "ratio": round(statistics.median(po) / statistics.median(dp), 3), "block_spread_ms": round(spread, 3),
                          "default_and_pose_only_same_track": same, "not_slower_beyond_spread": bool(saved > -spread),
                          "faster_beyond_spread": bool(saved > spread)}), flush=True)
        del trackers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
