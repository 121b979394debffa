"""What the per-Gaussian contribution pass costs beside the raster backward of the same frame.

On the headline scene (2.4 M Gaussians, 1080p, rgb: cfg5) and on cfg2 (376 k) a training frame is rendered; per block the frame
is rendered again and one backward consumes the preparation the forward left on the side stream (both untimed, the stream
drained behind them).  Then two windows are timed with device events: ``--reps`` calls of ``FrameRenderer.contributions`` back
to back, and as many calls of the same frame's raster backward (``backward(part=GS_BWD_RASTER)``: the launch whose
per-(Gaussian, pixel) work the pair pass forms a subset of).  Back to back, so that the host's enqueue latency of an idle
device is paid once per window and not once per call; behind a consumed preparation, so that every call of either kind
issues the same three small launches (stop keys, bucket scan, bucket fill) in front of its own kernels -- both figures
carry them, which is why they are larger than a call behind a fresh forward.  Median (min .. max) over the blocks of the
window's time per call.  Bytes moved are the algorithmic ones, counted from the frame's own counters (composited list
entries, buckets, Gaussians), over the 8.0 TB/s HBM peak:
  pair pass     : per composited list entry 4 (id) + 64 (record) + 16 (rectangle) + 4 (pair offset) read, 16 written; per
                  bucket 4 KiB of checkpoint lines read (the transmittance is one float of each 16-byte state);
  Gaussian pass : per Gaussian 16 (rectangle) + 4 (pair offset) read and 16 written; per pair 4 (stop key); per existing row
                  (= composited list entry) 16 read.
How the time splits between the two launches: a kernel trace of this script (profiles/contrib_cost.txt).

    python tools/contrib_cost.py [--blocks 15] [--reps 10] [--configs cfg5,cfg2]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussian import _lib  # noqa: E402
from gs_frame import FrameRenderer  # noqa: E402
from gs_scene import CONFIGS, make_camera, make_scene  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    """Microseconds per call of ``reps`` calls issued back to back."""
    tic, toc = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tic.record()
    for _ in range(reps):
        fn()
    toc.record()
    toc.synchronize()
    return tic.elapsed_time(toc) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="cfg5,cfg2")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    print(f"contribution pass against the raster backward of the same frame: microseconds per call, median (min .. max) over "
          f"{a.blocks} blocks of two windows of {a.reps} back-to-back calls, behind an untimed forward + backward")
    for name in a.configs.split(","):
        n, W, H, sh = CONFIGS[name]
        scene = make_scene(n, W, H, use_sh=sh)
        cam = make_camera(W, H)
        params = [torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
                  for x in (scene.pos, scene.quat, scene.scale, scene.opa, scene.rgb)]
        r = FrameRenderer(dev, max_pairs=1 << 22, training=True, auto_grow=True)
        grad = torch.randn(H, W, 3, device=dev)
        out = None
        for _ in range(3):  # warm-up: the workspace grows, the backward kernel is chosen, every shape has run once
            r.forward(*params, cam, training=True)
            c = r.contributions()
            out = r.backward(grad, out=out)
            st = r.stats()
        entries, buckets, pairs = r.composited_steps(), st.buckets, st.pairs
        t_c, t_b = [], []
        for _ in range(a.blocks):
            r.forward(*params, cam, training=True)
            r.backward(grad, out=out, part=_lib.GS_BWD_RASTER)
            torch.cuda.synchronize()
            t_c.append(timed(lambda: r.contributions(out=c), a.reps))
            t_b.append(timed(lambda: r.backward(grad, out=out, part=_lib.GS_BWD_RASTER), a.reps))
        pair_bytes = entries * (4 + 64 + 16 + 4 + 16) + buckets * 4096
        gauss_bytes = n * (16 + 4 + 16) + pairs * 4 + entries * 16
        med_c, med_b = statistics.median(t_c), statistics.median(t_b)
        rows = bool(r._frame.flags & _lib.GS_FRAME_BWD_ROWS)
        print(f"{name}: {n} Gaussians, {W} x {H}, {'SH' if sh else 'rgb'}; {st.visible} visible, {pairs} pairs, {entries} "
              f"composited list entries in {buckets} buckets; seen at 1/255: {int((c.views > 0).sum())}")
        print(f"  contributions (pair pass + Gaussian pass): {med_c:8.1f} ({min(t_c):.1f} .. {max(t_c):.1f}) us; "
              f"{(pair_bytes + gauss_bytes) / 1e6:.1f} MB moved = {(pair_bytes + gauss_bytes) / med_c / 1e6:.2f} TB/s = "
              f"{100 * (pair_bytes + gauss_bytes) / med_c / 1e-6 / HBM_PEAK:.1f} % of the HBM peak")
        print(f"  raster backward ({'row-layout' if rows else 'pixel'} kernel)       : {med_b:8.1f} ({min(t_b):.1f} .. "
              f"{max(t_b):.1f}) us; the pass costs {med_c / med_b:.2f} x the backward")


if __name__ == "__main__":
    main()
