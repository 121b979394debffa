"""The whole track / decide / seed / map loop on a synthetic sequence: a ``gs_scene.make_scene`` truth scene, N frames rendered
along an arc (image, and range = D / A where A >= 0.9), ``gs_slam.Slam`` over them.  Per frame: pose errors against the true
pose, keyframe flag, window, Gaussians added and pruned, milliseconds in track / overlap / seed / map / prune; at the end the
colour loss on each keyframe, right after its seeding and at the end of the run, and the worst pose error.

    python tools/slam_sequence.py [--frames 12] [--width 320 --height 240] [--gaussians 40000] [--step-deg 0.5 --step 0.02]
                                  [--map-iterations 120] [--overlap-min 0.9] [--carry-optimizer] [--prune-every K]
                                  [--prune-opa-min 0.005] [--prune-scale-max S] [--prune-unseen-every K]
                                  [--prune-unseen-w-min 0.00392] [--count-unseen]

``--count-unseen`` also reports, behind every keyframe's mapping steps (and prunes), how many Gaussians reach the weight
``--prune-unseen-w-min`` in no keyframe (``Trainer.contributions``: it renders every keyframe and leaves the fit alone).
"""
import argparse
import copy
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_frame import FrameRenderer  # noqa: E402
from gs_scene import make_camera, make_scene  # noqa: E402
from gs_slam import Slam, SlamOptions  # noqa: E402
from gs_track import so3_exp  # noqa: E402
from gs_train import ImageLoss  # noqa: E402


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--gaussians", type=int, default=40000)
    ap.add_argument("--step-deg", type=float, default=0.5)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--keyframe-every", type=int, default=SlamOptions().keyframe_every)
    ap.add_argument("--overlap-min", type=float, default=SlamOptions().overlap_min)
    ap.add_argument("--map-iterations", type=int, default=SlamOptions().map_iterations)
    # map edits that keep the optimizer state: off by default, as in SlamOptions
    ap.add_argument("--carry-optimizer", action="store_true")
    ap.add_argument("--prune-every", type=int, default=0)
    ap.add_argument("--prune-opa-min", type=float, default=SlamOptions().prune_opa_min)
    ap.add_argument("--prune-scale-max", type=float, default=None)
    ap.add_argument("--prune-unseen-every", type=int, default=0)
    ap.add_argument("--prune-unseen-w-min", type=float, default=SlamOptions().prune_unseen_w_min)
    ap.add_argument("--count-unseen", action="store_true")
    return ap


def run(a):
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    scene = make_scene(a.gaussians, W, H, seed=103)
    truth = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
             for x in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
    cam = make_camera(W, H, yaw_deg=2.0)
    cam.tran = np.array([0.03, -0.01, 0.2], np.float32)
    g = np.random.default_rng(211)
    axis, u = g.normal(size=3), g.normal(size=3)
    dR = so3_exp(axis / np.linalg.norm(axis) * math.radians(a.step_deg))
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * a.step - (dR @ t - t)
    poses = [(R, t)]
    for _ in range(a.frames - 1):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    renderer = FrameRenderer(dev, max_pairs=1 << 21, training=False, auto_grow=True, occlusion_cull=False)

    def posed(R, t):
        c = copy.copy(cam)
        c.rot, c.tran = np.asarray(R, np.float32), np.asarray(t, np.float32)
        return c

    def err(Ra, ta, Rb, tb):
        return float(np.linalg.norm(Ra - Rb) / math.sqrt(2.0)), float(np.linalg.norm(ta - tb))

    opts = SlamOptions(keyframe_every=a.keyframe_every, overlap_min=a.overlap_min, map_iterations=a.map_iterations,
                       carry_optimizer=a.carry_optimizer, prune_every=a.prune_every, prune_opa_min=a.prune_opa_min,
                       prune_scale_max=a.prune_scale_max, prune_unseen_every=a.prune_unseen_every,
                       prune_unseen_w_min=a.prune_unseen_w_min)
    slam = Slam(posed(*poses[0]), opts, dev)
    print(f"slam sequence: {a.gaussians} truth Gaussians, {W} x {H}, {a.frames} frames, {a.step_deg} degrees and {a.step} per "
          f"frame, keyframe_every {a.keyframe_every}, overlap_min {a.overlap_min}, map_iterations {a.map_iterations}, "
          f"carry_optimizer {a.carry_optimizer}, prune_every {a.prune_every} (opa_min {a.prune_opa_min}, scale_max "
          f"{a.prune_scale_max}), prune_unseen_every {a.prune_unseen_every} (w_min {a.prune_unseen_w_min:.5f}), defaults "
          f"otherwise")
    ev = FrameRenderer(dev, max_pairs=1 << 21, training=False, auto_grow=True)
    probe = ImageLoss(H, W, slam.opt.train.ssim_weight, dev)

    def colour_loss(k):
        image = ev.forward(*slam.params, slam.keyframes.cameras[k], training=False)[0]
        probe(image.contiguous(), slam.keyframes.images[k])
        return float(probe.values[0])

    seeded, worst = [], [0.0, 0.0]
    for f, (R, t) in enumerate(poses):
        img, _, d, al = renderer.forward(*truth, posed(R, t), training=False, aux=True)
        rng = torch.where(al >= 0.9, d / al.clamp_min(1e-3), torch.zeros_like(d)).contiguous()
        fr = slam.begin(img.contiguous().clone(), rng)
        if fr.keyframe:
            seeded.append(colour_loss(len(slam.keyframes) - 1))  # right after its seeding, before its mapping steps
        fr = slam.map(fr)
        e = err(fr.rot, fr.tran, R, t)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        ms = ", ".join(f"{k} {1e3 * fr.seconds[k]:.1f}" for k in ("track", "overlap", "seed", "map", "prune", "prune_unseen")
                       if k in fr.seconds)
        unseen = ""
        if a.count_unseen and fr.keyframe:
            c = slam.trainer.contributions(w_min=a.prune_unseen_w_min)
            unseen = f" unseen by every keyframe {int((c.views == 0).sum())}"
        print(f"  frame {f}: rotation error {e[0]:.3e} translation error {e[1]:.3e} keyframe {fr.keyframe} window {fr.window} "
              f"added {fr.added} pruned {fr.pruned} pruned_unseen {fr.pruned_unseen} Gaussians {slam.trainer.n_gaussians}"
              f"{unseen}; ms: {ms}")
    final = [colour_loss(k) for k in range(len(slam.keyframes))]
    for k, (s0, s1) in enumerate(zip(seeded, final)):
        print(f"  keyframe {k}: colour loss {s0:.5f} seeded -> {s1:.5f} at the end ({'below' if s1 < s0 else 'ABOVE'})")
    print(f"  worst pose error (rotation, translation): {worst[0]:.3e}, {worst[1]:.3e}; Gaussians at the end "
          f"{slam.trainer.n_gaussians}; optimizer step count {slam.trainer.optimizer.step_count} of {slam.i_iter} mapping steps")
    return dict(seeded=seeded, final=final, worst=worst, gaussians=slam.trainer.n_gaussians)


def main():
    a = parser().parse_args()
    return run(a)


if __name__ == "__main__":
    main()
