"""What the covisibility count costs: gs_view_overlap (two launches, timed with device events, no host read),
``gs_slam.KeyframeSet.overlap`` with its host read of the n + 2 counts, and the same count restated with torch operations on
the device (back-projection, one broadcast matmul against all views, comparisons over points x views, sums) -- at 640 x 480 and
1920 x 1080, strides 1 and 2, with 8, 64 and 256 views.  Median over 15 blocks of calls.

    python tools/overlap_cost.py [--blocks 15] [--calls 100]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_scene import Camera, make_camera  # noqa: E402
from gs_slam import KeyframeSet, view_overlap  # noqa: E402


def _origin(size):
    pad = (size + 15) // 16 * 16
    return (pad - size) // 2 - pad // 2


def torch_restatement(z, cam, rots, trans, focal, lo, hi, stride, near):
    """The count with torch operations (fp32 on the device) -> int64 [n + 2] on the device."""
    H, W = z.shape
    off = stride // 2
    zs = z[off::stride, off::stride]
    meas = torch.isfinite(zs) & (zs > 0)
    ys = torch.arange(off, H, stride, device=z.device, dtype=torch.float32)[:, None]
    xs = torch.arange(off, W, stride, device=z.device, dtype=torch.float32)[None, :]
    u = (xs + (_origin(W) + 0.5)) / float(cam.focal_x)
    v = (ys + (_origin(H) + 0.5)) / float(cam.focal_y)
    zc = torch.where(meas, zs, torch.zeros_like(zs)) / torch.sqrt(u * u + v * v + 1.0)
    rot = torch.from_numpy(np.asarray(cam.rot, np.float32)).to(z.device)
    tran = torch.from_numpy(np.asarray(cam.tran, np.float32)).to(z.device)
    p = (torch.stack([u * zc, v * zc, zc], -1).reshape(-1, 3) - tran) @ rot  # [L,3]
    q = torch.einsum("kij,lj->kli", rots, p) + trans[:, None, :]  # [n,L,3]
    qz = q[..., 2]
    a = focal[:, None, :] * q[..., :2]
    seen = (qz > near) & (a >= lo[:, None, :] * qz[..., None]).all(-1) & (a < hi[:, None, :] * qz[..., None]).all(-1)
    seen = seen & meas.reshape(1, -1)
    n_meas = meas.sum()
    return torch.cat([seen.sum(1), n_meas[None], (n_meas - seen.any(0).sum())[None]])


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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    print(f"covisibility count: microseconds per call, median (min .. max) over {a.blocks} blocks")
    for W, H in ((640, 480), (1920, 1080)):
        cam = make_camera(W, H, yaw_deg=3.0)
        cam.tran = np.array([0.1, -0.05, 0.2], np.float32)
        z = g.uniform(1.0, 6.0, (H, W)).astype(np.float32)
        z[g.uniform(size=(H, W)) < 0.1] = 0.0  # a tenth of the frame carries no measurement
        tz = torch.from_numpy(z).to(dev)
        ks = KeyframeSet(device=dev)
        img = torch.zeros((H, W, 3), device=dev)
        for k in range(256):  # views along an arc: from full overlap to none
            c = make_camera(W, H, yaw_deg=3.0 + 0.2 * k)
            c.tran = np.array([0.1 + 0.01 * k, -0.05, 0.2], np.float32)
            ks.add(Camera(W, H, c.focal_x, c.focal_y, c.rot, c.tran), img, tz)
        border, near = 0, 0.3
        for stride in (1, 2):
            for n in (8, 64, 256):
                rots = torch.from_numpy(np.stack([c.rot for c in ks.cameras[:n]]).astype(np.float32)).to(dev)
                trans = torch.from_numpy(np.stack([c.tran for c in ks.cameras[:n]]).astype(np.float32)).to(dev)
                focal = torch.tensor([[c.focal_x, c.focal_y] for c in ks.cameras[:n]], device=dev)
                lo = torch.tensor([[border + _origin(W), border + _origin(H)]] * n, dtype=torch.float32, device=dev)
                hi = torch.tensor([[W - border + _origin(W), H - border + _origin(H)]] * n, dtype=torch.float32, device=dev)
                sub = KeyframeSet(capacity=n, device=dev)
                for c in ks.cameras[:n]:
                    sub.add(c, img, tz)

                def kernel():
                    return view_overlap(tz, cam, sub.table, n, stride, near, border)

                def with_read():
                    return sub.overlap(tz, cam, stride, near, border)

                def restated():
                    return torch_restatement(tz, cam, rots, trans, focal, lo, hi, stride, near)

                got, ref = kernel().cpu().numpy(), restated().cpu().numpy()
                # (torch contracts and reorders: a few points on a border may fall the other way)
                diff = int(np.abs(got - ref).max())
                calls = a.calls
                heavy = max(2, calls // 20) if n * (H // stride) * (W // stride) > 5e7 else calls
                rows = [("gs_view_overlap (2 launches)", timed(kernel, a.blocks, calls)),
                        ("KeyframeSet.overlap (+ host read)", timed(with_read, a.blocks, calls)),
                        ("torch restatement", timed(restated, a.blocks, heavy))]
                print(f"{W} x {H}, stride {stride}, {n} views: {int(got[n])} measured lattice pixels, {int(got[n + 1])} seen by "
                      f"no view, max |count - torch count| {diff}")
                for label, (med, lo_, hi_) in rows:
                    print(f"    {label:36s} {med:10.1f} ({lo_:.1f} .. {hi_:.1f})")
                del rots, trans, focal
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
