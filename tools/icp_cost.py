#!/usr/bin/env python3
"""What the depth alignment costs and what it reaches (gs_icp_model_maps / gs_icp_step, csrc/icp.hip; gs_icp.IcpAligner;
gs_slam.SlamOptions.icp), one MI355X.  Three legs, JSON lines on stdout (profiles/icp.txt is this output with remarks):

  cost   at 160 x 120 (20,000 Gaussians), 640 x 480 (376,467) and 1920 x 1080 (2.4 M): us per gs_icp_model_maps, us per
         gs_icp_step pair at strides 4, 2 and 1, ms per whole align() with its single read -- and, from the same run, ms per
         Tracker.iteration and ms per aux forward at the same size.  Kernel legs: device events around blocks of K calls;
         legs that end in a host read: the host clock.  Warm-up first, then the legs interleaved in rounds; medians with the
         spread of the blocks.
  basin  start errors 0.5, 1, 2, 4 and 8 degrees (translation 0.04 per degree; the axis and direction of
         tests/track_ref.py::perturbed_start) on the analytic room corner of tests/icp_ref.py (the model given as the exact
         range map from the start pose; there is no Gaussian map of the corner, so only ICP runs there) and on the scene of
         tests/test_gpu_track.py (the model rendered from the start pose): end errors of the Tracker alone, ICP alone, and ICP
         then the Tracker, with the inlier shares and whether ICP was accepted.
  arc    the eight-frame arc of tests/test_gpu_slam.py through gs_slam.Slam with and without SlamOptions.icp: per-frame pose
         errors and seconds.

    python tools/icp_cost.py [--calls 200] [--rounds 5] [--warmup 10] [--legs cost,basin,arc] [--cases small,vga,1080p]
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))  # icp_ref (the corner), track_ref (the starts)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import icp_ref  # noqa: E402
from gs_frame import FrameRenderer  # noqa: E402
from gs_icp import IcpAligner, IcpOptions  # noqa: E402
from gs_scene import make_camera, make_scene  # noqa: E402
from gs_track import TrackOptions, Tracker  # noqa: E402
from track_ref import perturbed_start, pose_errors, so3_exp_series  # noqa: E402

CASES = [("small", 20_000, 160, 120, 103), ("vga", 376_467, 640, 480, 0), ("1080p", 2_400_000, 1920, 1080, 0)]
STARTS = [(d, 0.04 * d) for d in (0.5, 1.0, 2.0, 4.0, 8.0)]


def out(**kw):
    print(json.dumps(kw), flush=True)


def events_us(fn, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(k):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / k


def host_ms(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / k


def posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def scene_on(dev, n, W, H, seed):
    scene = make_scene(n, W, H, seed=seed) if seed else make_scene(n, W, H)
    cam = make_camera(W, H, yaw_deg=2.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    params = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
    return params, cam


def render(r, params, cam):
    img, _, d, a = r.forward(*params, cam, training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d)).contiguous()
    return img.contiguous().clone(), rng.clone(), d.contiguous().clone(), a.contiguous().clone()


def cost_leg(args, dev):
    import ctypes as C

    from gaussian import _lib

    for name, n, W, H, seed in CASES:
        if name not in args.cases.split(","):
            continue
        params, cam = scene_on(dev, n, W, H, seed)
        r = FrameRenderer(dev, max_pairs=1 << 22, training=False, occlusion_cull=False, auto_grow=True)
        R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
        R0, t0 = perturbed_start(R_true, t_true, angle_deg=0.5, shift=0.02)
        img, rng, _, _ = render(r, params, cam)
        _, _, d0, a0 = render(r, params, posed(cam, R0, t0))
        al = IcpAligner(cam, IcpOptions(), dev)
        vertex, normal = al.set_model(d0, a0, R0, t0)
        tr = Tracker(params, cam, TrackOptions(max_pairs=1 << 22), dev)
        state, log = al._dev[:16], al._dev[16:]
        eye, zero = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(0, 0, 0)
        stream = torch.cuda.current_stream().cuda_stream

        def step_fn(stride):
            ws = al._workspace(al._cam, stride)
            o = _lib.GsIcpOpts(stride, 0.2, 0.0, 6, 1e-6)

            def fn():  # (row 0 every time: the state keeps moving towards the answer, the work per call does not change)
                _lib.check(_lib.gs_icp_step(rng.data_ptr(), C.byref(al._cam), vertex.data_ptr(), normal.data_ptr(),
                                            C.byref(al._model[2]), C.byref(o), state.data_ptr(), log.data_ptr(), al._rows, 0,
                                            ws.data_ptr(), ws.numel(), stream), "gs_icp_step")
            return fn

        _lib.check(_lib.gs_icp_reset(state.data_ptr(), log.data_ptr(), al._rows, eye, zero, stream), "gs_icp_reset")
        pose_cam = posed(cam, R0, t0)
        kernel_legs = {"model_maps": lambda: al.set_model(d0, a0, R0, t0),
                       "step_stride4": step_fn(4), "step_stride2": step_fn(2), "step_stride1": step_fn(1),
                       "aux_forward": lambda: r.forward(*params, pose_cam, training=False, aux=True)}
        host_legs = {"align": lambda: al.align(rng), "tracker_iteration": lambda: tr.iteration(R0, t0, img, rng)}
        for f in list(kernel_legs.values()) + list(host_legs.values()):
            for _ in range(args.warmup):
                f()
        times = {k: [] for k in list(kernel_legs) + list(host_legs)}
        for _ in range(args.rounds):
            for k, f in kernel_legs.items():
                times[k].append(events_us(f, args.calls))
            for k, f in host_legs.items():
                times[k].append(host_ms(f, max(args.calls // 10, 5)))
        for k, v in times.items():
            unit = "ms" if k in host_legs else "us"
            out(case=name, what="cost", leg=k, width=W, height=H, gaussians=n, **{f"{unit}_median": round(statistics.median(v), 3),
                f"{unit}_min": round(min(v), 3), f"{unit}_max": round(max(v), 3)}, blocks=len(v))
        res = al.align(rng)
        e = pose_errors(res.rot, res.tran, R_true, t_true)
        out(case=name, what="cost_check", start=[round(x, 6) for x in pose_errors(R0, t0, R_true, t_true)],
            end=[float(f"{x:.3e}") for x in e], accepted=res.accepted, inliers=res.inliers, measured=res.measured,
            rmse=float(f"{res.rmse:.3e}"))
        del r, tr, al, params
        torch.cuda.empty_cache()


def basin_leg(dev):
    # ---- the analytic corner: exact maps, ICP alone
    cam = icp_ref.corner_camera()

    class Camera:
        rot, tran = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        focal_x = focal_y = cam.focal_x
        width, height = cam.width, cam.height

    al = IcpAligner(Camera(), IcpOptions(), dev)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    z = to_dev(icp_ref.corner_range(icp_ref.CORNER_ROT, icp_ref.CORNER_TRAN))
    for deg, shift in STARTS:
        R0, t0 = perturbed_start(icp_ref.CORNER_ROT, icp_ref.CORNER_TRAN, angle_deg=deg, shift=shift)
        al.set_model(to_dev(icp_ref.corner_range(R0, t0)), None, R0, t0)
        res = al.align(z)
        R, t = icp_ref.frame_pose(R0, t0, *res.relative)  # (also where ICP was declined: what it would have returned)
        e = pose_errors(R, t, icp_ref.CORNER_ROT, icp_ref.CORNER_TRAN)
        out(case="corner_160x120", what="basin", variant="icp", start_deg=deg, start_shift=shift,
            rot_err=float(f"{e[0]:.3e}"), tran_err=float(f"{e[1]:.3e}"),
            to_a_tenth=bool(e[0] <= 0.1 * math.radians(deg) and e[1] <= 0.1 * shift), accepted=res.accepted,
            inlier_share_first=round(res.log[0, 0] / max(res.log[0, 1], 1), 4),
            inlier_share_last=round(res.inliers / max(res.measured, 1), 4), rmse=float(f"{res.rmse:.3e}"))
    # ---- the scene of tests/test_gpu_track.py: the model rendered from the start pose
    params, cam = scene_on(dev, 20_000, 160, 120, 103)
    r = FrameRenderer(dev, max_pairs=1 << 19, training=False, occlusion_cull=False, auto_grow=True)
    img, rng, _, _ = render(r, params, cam)
    R_true, t_true = np.asarray(cam.rot, np.float64), np.asarray(cam.tran, np.float64)
    tr = Tracker(params, cam, TrackOptions(), dev)
    al = IcpAligner(cam, IcpOptions(), dev)
    for deg, shift in STARTS:
        R0, t0 = perturbed_start(R_true, t_true, angle_deg=deg, shift=shift)
        c0 = posed(cam, R0, t0)
        _, _, d0, a0 = render(r, params, c0)
        al.set_model(d0, a0, c0.rot.astype(np.float64), c0.tran.astype(np.float64))
        res = al.align(rng)
        Ri, ti = icp_ref.frame_pose(c0.rot.astype(np.float64), c0.tran.astype(np.float64), *res.relative)
        rows = {"icp": (Ri, ti)}
        tr.reset()
        alone = tr.track(img, rng, init=(R0, t0))
        rows["tracker"] = (alone.rot, alone.tran)
        tr.reset()
        both = tr.track(img, rng, init=(res.rot, res.tran) if res.accepted else (R0, t0))
        rows["icp_then_tracker"] = (both.rot, both.tran)
        for k, (R, t) in rows.items():
            e = pose_errors(R, t, R_true, t_true)
            out(case="test_scene_160x120", what="basin", variant=k, start_deg=deg, start_shift=shift,
                rot_err=float(f"{e[0]:.3e}"), tran_err=float(f"{e[1]:.3e}"),
                to_a_tenth=bool(e[0] <= 0.1 * math.radians(deg) and e[1] <= 0.1 * shift), icp_accepted=res.accepted,
                inlier_share_first=round(res.log[0, 0] / max(res.log[0, 1], 1), 4),
                inlier_share_last=round(res.inliers / max(res.measured, 1), 4), icp_rmse_first=float(
                    f"{math.sqrt(res.log[0, 2] / max(res.log[0, 0], 1)):.3e}"), icp_rmse=float(f"{res.rmse:.3e}"))


def arc_leg(dev):
    from gs_slam import Slam, SlamOptions

    params, cam = scene_on(dev, 20_000, 160, 120, 103)
    r = FrameRenderer(dev, max_pairs=1 << 19, training=False, occlusion_cull=False, auto_grow=True)
    g = np.random.default_rng(211)  # (the arc of tests/test_gpu_slam.py::_poses)
    axis = g.normal(size=3)
    axis /= np.linalg.norm(axis)
    dR = so3_exp_series(axis * math.radians(0.5))
    u = g.normal(size=3)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * 0.02 - (dR @ t - t)
    poses = [(R, t)]
    for _ in range(7):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    targets = [render(r, params, posed(cam, R, t))[:2] for R, t in poses]
    for variant, icp in (("without_icp", None), ("with_icp", IcpOptions()), ("without_icp_again", None)):
        slam = Slam(posed(cam, *poses[0]), SlamOptions(overlap_min=0.0, keyframe_every=3, icp=icp), dev)
        for f, ((R, t), (img, rng)) in enumerate(zip(poses, targets)):
            fr = slam.step(img, rng)
            e = pose_errors(fr.rot, fr.tran, R, t)
            row = dict(case="arc_160x120", what="arc", variant=variant, frame=f, keyframe=fr.keyframe,
                       rot_err=float(f"{e[0]:.3e}"), tran_err=float(f"{e[1]:.3e}"),
                       seconds={k: round(v, 4) for k, v in fr.seconds.items()})
            if fr.icp is not None:
                ie = pose_errors(fr.icp.rot, fr.icp.tran, R, t)
                row.update(icp_accepted=fr.icp.accepted, icp_rot_err=float(f"{ie[0]:.3e}"), icp_tran_err=float(f"{ie[1]:.3e}"),
                           icp_inlier_share=round(fr.icp.inliers / max(fr.icp.measured, 1), 4),
                           icp_rmse_first=float(f"{math.sqrt(fr.icp.log[0, 2] / max(fr.icp.log[0, 0], 1)):.3e}"),
                           icp_rmse=float(f"{fr.icp.rmse:.3e}"), icp_failed_solves=int((fr.icp.log[:, 36] != 0).sum()))
            out(**row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default="cost,basin,arc")
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("icp_cost.py measures on a HIP device; there is none")
    dev = torch.device("cuda:0")
    legs = args.legs.split(",")
    if "basin" in legs:
        basin_leg(dev)
    if "arc" in legs:
        arc_leg(dev)
    if "cost" in legs:
        cost_leg(args, dev)


if __name__ == "__main__":
    main()
