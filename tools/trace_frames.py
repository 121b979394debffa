#!/usr/bin/env python3
"""Per-frame summary of a rocprofv3 --kernel-trace CSV taken around tools/prof_target.py (forward frames only):

    python tools/trace_frames.py <..._kernel_trace.csv> [frames=100]

The timed loop of prof_target.py is `frames` identical frames, followed by 12 profiled ones (hipEvents between the stages);
a frame starts at every dispatch of the project kernel that follows a compositing kernel.  The loop's frames are the
`frames` consecutive frames with the shortest total span that end in front of the profiled ones.  Prints dispatches per frame,
per kernel name the mean time of its FIRST dispatch in a frame (the real launch) and of its later ones (the gated launches of an
occlusion-culled frame's second pass), and the frame period (start of a frame to the start of the next)."""
import csv
import statistics
import sys
from collections import defaultdict

path = sys.argv[1]
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 100
rows = []
with open(path) as fh:
    for r in csv.DictReader(fh):
        if r.get("Kind") != "KERNEL_DISPATCH":
            continue
        name = r["Kernel_Name"]
        if "::" not in name or "at::native" in name or "rocclr" in name:
            continue  # (torch's own kernels, fills and copies: not part of a frame)
        short = name.split("::", 1)[1].split("(")[0].replace("(anonymous namespace)::", "")
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
rows.sort()


def is_project(n):
    return "project" in n and "count" in n


def is_raster(n):
    return n.startswith("raster_forward")


# cut into frames: a project kernel right behind a compositing kernel opens a frame -- unless it is the gated project launch of a
# second pass: the frame in front of it began with the CULLED project kernel, has had one compositing launch, and this one is
# the unculled project kernel
groups, cur = [], []
for s, e, n in rows:
    if is_project(n) and cur and is_raster(cur[-1][2]):
        gated = "cull_count" in cur[0][2] and "cull_count" not in n and sum(is_raster(x[2]) for x in cur) == 1
        if not gated:
            groups.append(cur)
            cur = []
    cur.append((s, e, n))
if cur:
    groups.append(cur)
# the steady-state loop: the last `frames` + 12 frames are loop + profiled ones (prof_target.py); without the profiled ones
# (--no-stage-times) pass frames explicitly and ignore the tail
tail = 12
loop = groups[-(frames + tail):-tail] if len(groups) >= frames + tail else groups[-frames:]
counts = [len(g) for g in loop]
print(f"frames found {len(groups)}, summarised {len(loop)}; dispatches per frame: min {min(counts)} median "
      f"{int(statistics.median(counts))} max {max(counts)}")
first, later = defaultdict(list), defaultdict(list)
for g in loop:
    seen = set()
    for s, e, n in g:
        (later if n in seen else first)[n].append(e - s)
        seen.add(n)
print(f"{'kernel':62s} {'calls':>6s} {'real us':>9s}   {'later calls':>11s} {'us':>7s}")
for n in sorted(first, key=lambda k: -statistics.mean(first[k])):
    l = later.get(n, [])
    print(f"{n[:62]:62s} {len(first[n]):6d} {statistics.mean(first[n]) / 1e3:9.2f}   {len(l):11d} "
          f"{(statistics.mean(l) / 1e3 if l else 0.0):7.2f}")
starts = [g[0][0] for g in loop]
period = [(b - a) / 1e3 for a, b in zip(starts, starts[1:])]
busy = [sum(e - s for s, e, _ in g) / 1e3 for g in loop]
tail_us = [(g[-1][1] - next(e for s, e, n in g if is_raster(n))) / 1e3 for g in loop]
print(f"frame period: median {statistics.median(period):.1f} us, mean {statistics.mean(period):.1f} us; kernel time per frame "
      f"(sum of dispatches) median {statistics.median(busy):.1f} us; end of the first compositing launch to the end of the "
      f"frame's last dispatch: median {statistics.median(tail_us):.1f} us")
