"""What keyframe eviction costs: one gs_view_redundancy call (two launches, timed with device events, no host read), a full
``gs_slam.KeyframeSet.redundancy()`` pass over 256 keyframes with its one host read, and beside them one gs_view_overlap call on
the same inputs and one mapping step (``Trainer.train_step``) of the map seeded from the same range map -- 640 x 480, lattice
stride 2.  Median over the blocks of calls.

    python tools/evict_cost.py [--blocks 15] [--calls 100] [--views 256]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python tools/evict_cost.py --blocks 2 --calls 20
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_scene import Camera, make_camera  # noqa: E402
from gs_seed import seed_from_depth  # noqa: E402
from gs_slam import KeyframeSet, _map_train_options, view_overlap, view_redundancy  # noqa: E402
from gs_train import Trainer  # noqa: E402


def timed(fn, blocks, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tic.record()
        for _ in range(calls):
            fn()
        toc.record()
        toc.synchronize()
        out.append(tic.elapsed_time(toc) * 1000.0 / calls)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--views", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    W, H, stride, near, border, n = 640, 480, 2, 0.3, 0, a.views
    cam = make_camera(W, H, yaw_deg=3.0)
    cam.tran = np.array([0.1, -0.05, 0.2], np.float32)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = (3.0 + 0.5 * np.sin(xs / 40.0) * np.cos(ys / 30.0)).astype(np.float32)  # a smooth surface ...
    z[g.uniform(size=(H, W)) < 0.1] = 0.0  # ... a tenth of which carries no measurement
    tz = torch.from_numpy(z).to(dev)
    img = torch.from_numpy(g.uniform(0.2, 0.8, (H, W, 3)).astype(np.float32)).to(dev)
    ks = KeyframeSet(capacity=n, device=dev)
    for k in range(n):  # views along an arc: from full overlap to none
        c = make_camera(W, H, yaw_deg=3.0 + 0.2 * k)
        c.tran = np.array([0.1 + 0.01 * k, -0.05, 0.2], np.float32)
        ks.add(Camera(W, H, c.focal_x, c.focal_y, c.rot, c.tran), img, tz)
    mid = n // 2
    hist = view_redundancy(tz, ks.cameras[mid], ks.table, n, mid, stride, near, border).cpu().numpy()
    counts = view_overlap(tz, ks.cameras[mid], ks.table, n, stride, near, border).cpu().numpy()
    print(f"keyframe eviction, {W} x {H}, stride {stride}, {n} keyframes: microseconds, median (min .. max) over {a.blocks} blocks "
          f"of {a.calls} calls")
    print(f"    keyframe {mid}: {int(hist[8])} measured lattice pixels, histogram {hist[:8].tolist()}; gs_view_overlap's own row "
          f"{int(counts[mid])}, seen by no view {int(counts[n + 1])}")
    out = torch.empty(9, dtype=torch.int64, device=dev)
    rows = [("gs_view_redundancy (2 launches)", timed(lambda: view_redundancy(tz, ks.cameras[mid], ks.table, n, mid, stride, near,
                                                                           border, out=out), a.blocks, a.calls)),
            # near = 100: no view sees anything, no wave can leave the view loop early -- the longest a call takes
            ("    ... nothing seen (near = 100)", timed(lambda: view_redundancy(tz, ks.cameras[mid], ks.table, n, mid, stride,
                                                                                 100.0, border, out=out), a.blocks, a.calls)),
            ("gs_view_overlap, same inputs", timed(lambda: view_overlap(tz, ks.cameras[mid], ks.table, n, stride, near, border),
                                                   a.blocks, a.calls))]
    passes = max(1, a.calls // 20)
    rows.append((f"KeyframeSet.redundancy(), {n} calls + host read", timed(lambda: ks.redundancy(stride, near, border), a.blocks,
                                                                          passes)))
    wall = []
    for _ in range(max(3, a.blocks // 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ks.redundancy(stride, near, border)
        wall.append((time.perf_counter() - t0) * 1e6)
    rows.append(("    ... wall clock of one pass", (statistics.median(wall), min(wall), max(wall))))
    rows.append(("    ... a pass in which nothing is seen (near = 100)", timed(lambda: ks.redundancy(stride, 100.0, border),
                                                                               a.blocks, passes)))
    # one mapping step of the map this range map seeds (the loop's own seed and train options), on the first keyframe
    params = seed_from_depth(img, tz, ks.cameras[0], color_dim=3)
    tr = Trainer(params, [ks.cameras[0]], [img], _map_train_options(), max_pairs=1 << 21, depths=[tz])
    step = [0]

    def map_step():
        tr.train_step(step[0], 0)
        step[0] += 1

    rows.append((f"one mapping step, {tr.n_gaussians} Gaussians", timed(map_step, a.blocks, max(2, a.calls // 5))))
    for label, (med, lo_, hi_) in rows:
        print(f"    {label:48s} {med:12.1f} ({lo_:.1f} .. {hi_:.1f})")
    per_kf = rows[3][1][0] / n  # (the pass with its host read; the mapping step is the last row)
    print(f"    per keyframe of the pass: {per_kf:.1f} us = {per_kf / rows[-1][1][0]:.3f} mapping steps")


if __name__ == "__main__":
    main()
