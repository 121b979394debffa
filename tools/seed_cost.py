"""What seeding from an RGB-D frame costs at 1080p: gs_seed_classify + gs_seed_apply (three launches, timed with device events,
no host read in between: the rows go into arrays of sufficient capacity), ``gs_seed.seed_from_depth`` end to end (with its host
read of the count and the allocation of the new arrays), and the same step restated with torch operations on the device (mask,
``nonzero``, gathers, elementwise arithmetic, ``stack``) -- for stride 1 and 2, an empty model (no maps: every measured pixel)
and a half-explained one (maps that leave about half of the measured pixels open).  Median over 15 blocks of 400 calls
(12 - 190 ms of device time per block).

    python tools/seed_cost.py [--blocks 15] [--calls 400]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gs_geometry import TileGrid  # noqa: E402
from gs_scene import make_camera  # noqa: E402
from gs_seed import DEFAULTS, seed_apply, seed_classify, seed_from_depth, seed_options  # noqa: E402


def torch_restatement(img, z, cam, maps, stride, o):
    """The step with torch operations (fp32 on the device), returning the five new tensors."""
    H, W = z.shape
    off = stride // 2
    zs = z[off::stride, off::stride]
    sel = torch.isfinite(zs) & (zs > 0)
    if maps is not None:
        D, A = (m[off::stride, off::stride] for m in maps)
        sel = sel & ((A < o["alpha_thresh"]) | (zs * A < (1.0 - o["front_rel"]) * D))
    iy, ix = torch.nonzero(sel, as_tuple=True)  # (synchronises)
    y, x = iy * stride + off, ix * stride + off
    rng = z[y, x]
    grid = TileGrid(W, H, float(cam.focal_x), float(cam.focal_y))
    top, left = grid.crop_offsets()
    u = (x + (left - grid.padded_width / 2 + 0.5)) / float(cam.focal_x)
    v = (y + (top - grid.padded_height / 2 + 0.5)) / float(cam.focal_y)
    zc = rng / torch.sqrt(u * u + v * v + 1.0)
    rot = torch.from_numpy(np.asarray(cam.rot, np.float32)).to(z.device)
    tran = torch.from_numpy(np.asarray(cam.tran, np.float32)).to(z.device)
    pos = (torch.stack([u * zc, v * zc, zc], 1) - tran) @ rot
    sigma = o["scale_factor"] * stride * zc / ((float(cam.focal_x) + float(cam.focal_y)) / 2)
    scale = (sigma - 1e-4).clamp_min(0)[:, None].expand(-1, 3).contiguous()
    n = pos.shape[0]
    quat = torch.zeros(n, 4, device=z.device)
    quat[:, 0] = 1.0
    opa = torch.full((n,), float(np.log(o["opa_init"] / (1 - o["opa_init"]))), device=z.device)
    c = img[y, x].clamp(1 / 512, 1 - 1 / 512)
    return pos, quat, scale, opa, torch.log(c / (1 - c))


def timed(fn, blocks, calls):
    for _ in range(5):
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
    ap.add_argument("--calls", type=int, default=400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    cam = make_camera(W, H, yaw_deg=12.0)
    cam.tran = np.array([0.3, -0.1, 0.2], np.float32)
    g = np.random.default_rng(0)
    z = g.uniform(0.5, 10.0, (H, W)).astype(np.float32)
    z[g.uniform(size=(H, W)) < 0.1] = 0.0  # a tenth of the frame carries no measurement
    A = np.where(g.uniform(size=(H, W)) < 0.5, 0.98, 0.05).astype(np.float32)  # half of the frame is explained
    D = (A * z).astype(np.float32)
    tz, tA, tD = (torch.from_numpy(x).to(dev) for x in (z, A, D))
    img = torch.from_numpy(g.uniform(0, 1, (H, W, 3)).astype(np.float32)).to(dev)
    o = dict(DEFAULTS)
    print(f"seeding at {W} x {H}: microseconds per call, median (min .. max) over {a.blocks} blocks of {a.calls} calls")
    for stride in (1, 2):
        for name, maps in (("empty model", None), ("half-explained model", (tD, tA))):
            opts = seed_options(stride=stride)
            counts, ws = seed_classify(tz, maps, opts)
            n, n_meas = (int(v) for v in counts.tolist())
            out = [torch.empty((n,) + s, device=dev) for s in ((3,), (4,), (3,), (), (3,))]

            def pair():
                c, w = seed_classify(tz, maps, opts)  # (allocates its small workspace through torch's caching allocator)
                seed_apply(img, tz, cam, opts, out, 0, c, w)

            def surface():
                return seed_from_depth(img, tz, cam, rendered=maps, stride=stride)

            def restated():
                return torch_restatement(img, tz, cam, maps, stride, o)

            ref, got = restated(), surface()
            assert got[0].shape[0] == n == ref[0].shape[0]
            dpos = float((got[0] - ref[0]).abs().max())
            # bytes the pair has to move: the lattice's range (+ two maps), and per selected pixel its range and colour again
            # and the 56 bytes of its rows
            lattice = (-(-(H - stride // 2) // stride)) * (-(-(W - stride // 2) // stride))
            nbytes = lattice * 4 * (3 if maps is not None else 1) + n * (4 + 12 + 56)
            rows = [("classify + apply (3 launches)", timed(pair, a.blocks, a.calls)),
                    ("seed_from_depth (+ host read, allocation)", timed(surface, a.blocks, a.calls)),
                    ("torch restatement", timed(restated, a.blocks, a.calls))]
            print(f"stride {stride}, {name}: {n} selected of {n_meas} measured lattice pixels; {nbytes / 1e6:.1f} MB needed; "
                  f"max |pos - torch pos| {dpos:.2e}")
            for label, (med, lo, hi) in rows:
                extra = f"  = {nbytes / med / 1e6:.2f} TB/s on the needed bytes" if label.startswith("classify") else ""
                print(f"    {label:44s} {med:9.1f} ({lo:.1f} .. {hi:.1f}){extra}")


if __name__ == "__main__":
    main()
