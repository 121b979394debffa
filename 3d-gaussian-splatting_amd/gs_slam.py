"""Mapping an RGB-D sequence: keyframes, their covisibility, and the track -> decide -> seed -> map loop.

``Slam(camera).step(image, range_map)`` takes the frames of a depth camera one at a time.  The first frame founds the map
(``gs_seed.seed_from_depth`` into an empty model, a ``gs_train.Trainer`` on that one view).  Every later frame is tracked
against the frozen map (``gs_track.Tracker``), then asked the covisibility question -- of the surface points this frame
measured, how many does each keyframe see? (``gs_view_overlap``, csrc/overlap.hip: one call, one host read) -- and becomes a
keyframe when the last keyframe sees too few of them or too many frames have passed.  A keyframe is added to the running fit
(``Trainer.add_view``), seeds Gaussians where the map does not explain it (``Trainer.seed_from_view``) and is optimised
together with the keyframes that share the most points with it.  A frame that is no keyframe leaves the map and the
optimizer state untouched, bit for bit.

rgb maps only.  With ``SlamOptions.icp`` every frame after the first is first aligned to the map's rendered depth by
point-to-plane ICP (``gs_icp.IcpAligner``) and the tracker starts from the aligned pose where the alignment is accepted.  By
default a keyframe's pose is fixed once set.  With ``SlamOptions.refine_poses`` the mapping steps of a
keyframe also refine the poses of its window (``Trainer.free_pose``: the fused step's pose variant,
gs_frame_backward_adam_pose, delivers the pose gradient of every step, the Tracker's pose optimizer takes it) -- every view of
the window except keyframe 0, which fixes the gauge; ``KeyframeSet.set_pose`` carries the result into the view table and the
tracker's motion history starts from the refined pose.  By default the keyframe set only grows -- ``KeyframeSet.add`` raises
when it is full (256 views).  With ``SlamOptions.max_keyframes`` the set is capped: a keyframe that arrives at the cap first
evicts the most redundant one -- the keyframe with the largest share of its own measured points seen by at least
``evict_seen_by`` other keyframes (``gs_view_redundancy``, csrc/redundancy.hip: one call per keyframe, one host read;
``select_eviction``) -- from the set (``KeyframeSet.remove``) and from the running fit (``Trainer.remove_view``); the Gaussians it
seeded stay.  There is no loop closure and ``adaptive_control`` is never called.

With ``SlamOptions.gate_map`` (off by default; it needs a gated tracker) a keyframe after the first reaches the trainer
through the tracker's median gate: the frozen map rendered once at the tracked pose, ``gs_train.GateMask`` on it, the range map
without the rejected measurements and the 0 / 1 colour weight into ``Trainer.add_view(..., weight=)`` -- what the tracker
rejected is neither seeded nor fitted.

Two options edit the map without resetting Adam, both off by default.  ``SlamOptions.carry_optimizer``: a keyframe's seeding
keeps the old rows' moments and the step count (``Trainer.seed_from_view(carry_state=True)``) instead of starting a fresh
optimizer for the whole map.  ``SlamOptions.prune_every`` = k: behind the mapping steps of every k-th keyframe the Gaussians
whose opacity training drove below ``prune_opa_min`` (or whose extent reached ``prune_scale_max``) are removed
(``Trainer.prune``, csrc/map_edit.hip: one compaction of parameters, moments and statistic), before the tracker is bound to
the map.
"""
from __future__ import annotations

import copy
import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import gs_seed
from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace
from gs_geometry import pose64, posed, principal_point_offset
from gs_icp import IcpAligner, IcpOptions, IcpResult
from gs_track import _SH_REFUSAL, TrackOptions, TrackResult, Tracker
from gs_train import GateMask, TrainOptions, Trainer

GS_OVERLAP_MAX_VIEWS = _lib.GS_OVERLAP_MAX_VIEWS
GS_REDUNDANCY_BINS = _lib.GS_REDUNDANCY_BINS


def view_overlap(range_map: torch.Tensor, camera, table: torch.Tensor, n_views: int, stride: int = 1, near: float = 0.3,
                 border: int = 0, table_pp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gs_view_overlap`` (include/gs_abi.h) -> counts [n_views + 2] int64 on the device: per view the measured lattice pixels
    of ``range_map`` whose surface point the view sees, then the measured lattice pixels, then those no view sees.  ``table``
    is the device array of view rows [>= n_views, 16] float32 (``KeyframeSet.table``); ``camera`` the frame's posed camera.
    No host synchronisation.  The rows of ``table`` are not validated here (``view_row`` does that when a row is made), and
    a ``border`` that leaves nothing of a view -- 2 border >= its width or height -- is NOT refused by this call: the sizes are
    in device memory.  ``KeyframeSet.overlap`` holds the border against its smallest view.

    Off-centre principal points: ``camera``'s own offset is honoured (``gs_geometry.principal_point_offset``); the views'
    offsets come as ``table_pp`` [>= n_views, 2] float32 on the device, row k = (dx_k, dy_k) in pixels
    (``KeyframeSet.table_pp``; None: no view has one).  With no offset anywhere the call is ``gs_view_overlap`` itself."""
    require_hip(range_map.device, "the overlap count")
    cam = gs_seed.seed_camera(camera)
    check_tensor("range_map", range_map, (cam.height, cam.width))
    check_tensor("table", table, rows_min=n_views, tail=(16,))
    opts = _lib.GsOverlapOpts(int(stride), float(near), int(border))
    ws = workspace(_lib.gs_view_overlap_workspace_bytes(cam.height, cam.width, max(int(stride), 1),
                                                        min(max(int(n_views), 1), GS_OVERLAP_MAX_VIEWS)), range_map.device)
    counts = torch.empty(max(int(n_views), 0) + 2, dtype=torch.int64, device=range_map.device)
    tail = (int(n_views), C.byref(opts), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    if table_pp is not None or principal_point_offset(camera) != (0.0, 0.0):
        if table_pp is not None:
            check_tensor("table_pp", table_pp, rows_min=n_views, tail=(2,), device=table.device)
        _lib.call("gs_view_overlap_pp", range_map.data_ptr(), C.byref(gs_seed.seed_camera_pp(camera)), table.data_ptr(),
                  table_pp.data_ptr() if table_pp is not None else None, *tail)
    else:
        _lib.call("gs_view_overlap", range_map.data_ptr(), C.byref(cam), table.data_ptr(), *tail)
    return counts


def view_redundancy(range_map: torch.Tensor, camera, table: torch.Tensor, n_views: int, self_index: int = -1, stride: int = 1,
                    near: float = 0.3, border: int = 0, table_pp: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gs_view_redundancy`` (include/gs_abi.h) -> hist [GS_REDUNDANCY_BINS + 1] int64 on the device: of the measured lattice
    pixels of ``range_map`` -- one view's own range map, ``camera`` its posed camera -- how many are seen by exactly 0, 1, ..., 6
    and by 7 or more of the rows of ``table`` other than row ``self_index`` (-1: no row is left out), then how many there are.
    The decisions are ``gs_view_overlap``'s, the checks ``view_overlap``'s: the rows of ``table`` are not validated here and a
    ``border`` that leaves nothing of a view is not refused.  No host synchronisation.  ``out``: a contiguous int64 tensor of
    nine elements on the device to write into (a row of a larger tensor: a caller collects many results and reads once);
    ``ws``: a uint8 workspace of at least ``gs_view_redundancy_workspace_bytes`` to share between stream-ordered calls.
    ``table_pp`` and ``camera``'s own principal-point offset as in ``view_overlap``."""
    require_hip(range_map.device, "the redundancy count")
    cam = gs_seed.seed_camera(camera)
    check_tensor("range_map", range_map, (cam.height, cam.width))
    check_tensor("table", table, rows_min=n_views, tail=(16,))
    opts = _lib.GsOverlapOpts(int(stride), float(near), int(border))
    if ws is None:
        ws = workspace(_lib.gs_view_redundancy_workspace_bytes(cam.height, cam.width, max(int(stride), 1)), range_map.device)
    if out is None:
        out = torch.empty(GS_REDUNDANCY_BINS + 1, dtype=torch.int64, device=range_map.device)
    elif not (out.dtype == torch.int64 and out.is_contiguous() and out.numel() == GS_REDUNDANCY_BINS + 1
              and out.device == range_map.device):
        raise ValueError(f"out must be a contiguous int64 tensor of {GS_REDUNDANCY_BINS + 1} elements on the range map's device")
    tail = (int(n_views), int(self_index), C.byref(opts), out.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    if table_pp is not None or principal_point_offset(camera) != (0.0, 0.0):
        if table_pp is not None:
            check_tensor("table_pp", table_pp, rows_min=n_views, tail=(2,), device=table.device)
        _lib.call("gs_view_redundancy_pp", range_map.data_ptr(), C.byref(gs_seed.seed_camera_pp(camera)), table.data_ptr(),
                  table_pp.data_ptr() if table_pp is not None else None, *tail)
    else:
        _lib.call("gs_view_redundancy", range_map.data_ptr(), C.byref(cam), table.data_ptr(), *tail)
    return out


def view_row(camera) -> np.ndarray:
    """A camera as one 64-byte row of the view table (``struct gs_seed_camera``), validated: ``gs_view_overlap`` cannot
    check rows that live in device memory, so the owner of the table does when it appends one."""
    cam = gs_seed.seed_camera(camera)
    _lib.call("gs_view_overlap_check_view", C.byref(cam), 0)
    return np.frombuffer(bytes(cam), np.float32).copy()


class KeyframeSet:
    """The keyframes of a mapping run: posed cameras, colour targets, range maps, and the device table of their 64-byte
    rows that ``gs_view_overlap`` reads.  ``add`` raises ``RuntimeError`` once ``capacity`` keyframes are held (at most
    GS_OVERLAP_MAX_VIEWS = 256); the set itself never evicts: its owner asks ``redundancy`` which keyframe measured the least
    that the others do not see, and calls ``remove``.  ``ids``: a list parallel to ``cameras``, the keyframes' stable ids
    0, 1, 2, ... in order of addition, never reused -- positions shift when a keyframe is removed, ids do not."""

    def __init__(self, capacity: int = GS_OVERLAP_MAX_VIEWS, device="cuda"):
        if not 1 <= int(capacity) <= GS_OVERLAP_MAX_VIEWS:
            raise ValueError(f"capacity must lie in [1, {GS_OVERLAP_MAX_VIEWS}]")
        self.capacity = int(capacity)
        self.cameras, self.images, self.ranges = [], [], []
        self.table = torch.zeros((self.capacity, 16), dtype=torch.float32, device=device)
        # the views' principal-point offsets (dx_k, dy_k), a table beside the 64-byte rows; handed to the count only once a
        # keyframe has one (a set of centred cameras runs the kernel it always ran, on the rows it always read)
        self.table_pp = torch.zeros((self.capacity, 2), dtype=torch.float32, device=device)
        self._offsets = []
        self._min_size = None
        self.ids: List[int] = []
        self._next_id = 0

    def __len__(self) -> int:
        return len(self.cameras)

    @property
    def n_added(self) -> int:
        """Keyframes ever added (the next id): ``len`` without removals."""
        return self._next_id

    def add(self, camera, image: torch.Tensor, range_map: torch.Tensor) -> int:
        """Appends a keyframe -> its index.  The row is validated on the host and written with one 64-byte copy."""
        n = len(self.cameras)
        if n >= self.capacity:
            raise RuntimeError(f"the keyframe set is full ({self.capacity} views); there is no eviction")
        row = view_row(camera)
        off = principal_point_offset(camera)
        self.table[n].copy_(torch.from_numpy(row))
        self.table_pp[n].copy_(torch.tensor(off, dtype=torch.float32))
        self._offsets.append(off)
        self.cameras.append(copy.copy(camera))
        self.images.append(image)
        self.ranges.append(range_map)
        self.ids.append(self._next_id)
        self._next_id += 1
        size = min(int(camera.width), int(camera.height))
        self._min_size = size if self._min_size is None else min(self._min_size, size)
        return n

    def remove(self, index: int):
        """Deletes the keyframe at position ``index``: the lists drop the entry, rows index + 1 .. n - 1 of ``table`` and
        ``table_pp`` move up by one (a device copy through a temporary; the freed last row is zeroed), every later keyframe's
        position falls by one and its id stays.  ``add`` works again on a set that was full."""
        n = len(self.cameras)
        index = int(index)
        if not 0 <= index < n:
            raise IndexError(f"no keyframe {index}")
        for t in (self.table, self.table_pp):
            if index + 1 < n:
                t[index:n - 1].copy_(t[index + 1:n].clone())
            t[n - 1].zero_()
        for lst in (self.cameras, self.images, self.ranges, self.ids, self._offsets):
            del lst[index]
        self._min_size = min((min(int(c.width), int(c.height)) for c in self.cameras), default=None)

    def set_pose(self, index: int, rot, tran):
        """Replaces the pose of keyframe ``index`` (a mapper refined it): the camera by a copy with (rot, tran) in float32,
        its 64-byte row of the device table by the validated row of that copy."""
        if not 0 <= int(index) < len(self.cameras):
            raise IndexError(f"no keyframe {index}")
        cam = posed(self.cameras[index], rot, tran)
        row = view_row(cam)  # (validated before anything is written)
        self.table[index].copy_(torch.from_numpy(row))
        self.cameras[index] = cam

    def overlap(self, range_map: torch.Tensor, camera, stride: int = 1, near: float = 0.3, border: int = 0) -> np.ndarray:
        """counts [len + 2] int64 on the host (``view_overlap``): the one host read of a frame's keyframe decision."""
        if not self.cameras:
            raise RuntimeError("the keyframe set is empty")
        if 2 * int(border) >= self._min_size:
            raise RuntimeError(f"border {border} leaves nothing of a {self._min_size}-pixel keyframe")
        table_pp = self.table_pp if any(o != (0.0, 0.0) for o in self._offsets) else None
        return view_overlap(range_map, camera, self.table, len(self.cameras), stride, near, border, table_pp).cpu().numpy()

    def redundancy(self, stride: int = 1, near: float = 0.3, border: int = 0) -> np.ndarray:
        """hists [len, GS_REDUNDANCY_BINS + 1] int64 on the host: row k is ``view_redundancy`` of keyframe k's own raw range
        map and camera against the other keyframes (``self_index`` = k).  One call per keyframe into one device tensor
        through one workspace, stream-ordered; one host read at the end.  ``table_pp`` is honoured as ``overlap`` does."""
        if not self.cameras:
            raise RuntimeError("the keyframe set is empty")
        if 2 * int(border) >= self._min_size:
            raise RuntimeError(f"border {border} leaves nothing of a {self._min_size}-pixel keyframe")
        table_pp = self.table_pp if any(o != (0.0, 0.0) for o in self._offsets) else None
        n = len(self.cameras)
        hists = torch.empty((n, GS_REDUNDANCY_BINS + 1), dtype=torch.int64, device=self.table.device)
        nbytes = max(int(_lib.gs_view_redundancy_workspace_bytes(int(c.height), int(c.width), max(int(stride), 1)))
                     for c in self.cameras)
        ws = workspace(nbytes, self.table.device)
        for k in range(n):
            view_redundancy(self.ranges[k], self.cameras[k], self.table, n, k, stride, near, border, table_pp, out=hists[k],
                            ws=ws)
        return hists.cpu().numpy()


def select_keyframes(counts: Sequence[int], measured: int, k: int, min_share: float) -> List[int]:
    """The up to ``k`` views with the highest counts among those with count >= min_share x measured, highest first; ties go
    to the higher index (the more recent keyframe).  No randomness."""
    floor = float(min_share) * float(measured)
    ok = [(int(c), i) for i, c in enumerate(counts) if int(c) >= floor]
    ok.sort(key=lambda ci: (-ci[0], -ci[1]))
    return [i for _, i in ok[:max(int(k), 0)]]


def select_eviction(hists, seen_by: int, protected: Sequence[int]) -> Optional[int]:
    """The keyframe to evict -> its position, or None when every position is protected.  ``hists`` [K, 9]: row k the
    histogram ``KeyframeSet.redundancy`` gives for keyframe k.  The score of row k is the share of its measured points that at
    least ``seen_by`` other keyframes see, sum(hists[k, seen_by:8]) / hists[k, 8]; a row that measured nothing scores 1.  The
    unprotected position with the highest score goes; ties go to the lower position (the older keyframe).  Scores are compared
    as exact fractions, by cross-multiplication of integers: ties are real ties.  No randomness."""
    seen_by = int(seen_by)
    if not 1 <= seen_by <= GS_REDUNDANCY_BINS - 1:
        raise ValueError(f"seen_by must lie in [1, {GS_REDUNDANCY_BINS - 1}]")
    barred = {int(p) for p in protected}
    best, best_num, best_den = None, 0, 1
    for k, row in enumerate(hists):
        if k in barred:
            continue
        num, den = sum(int(v) for v in row[seen_by:GS_REDUNDANCY_BINS]), int(row[GS_REDUNDANCY_BINS])
        if den == 0:
            num, den = 1, 1
        if best is None or num * best_den > best_num * den:  # (strictly higher: a tie keeps the lower position)
            best, best_num, best_den = k, num, den
    return best


def is_keyframe(count_last: int, measured: int, frames_since: int, overlap_min: float, every: int) -> bool:
    """A frame becomes a keyframe when the last keyframe sees less than ``overlap_min`` of its measured points, or
    ``every`` frames have passed since that keyframe."""
    return bool(int(count_last) < float(overlap_min) * float(measured) or int(frames_since) >= int(every))


def _map_train_options() -> TrainOptions:
    return TrainOptions(n_iters_warmup=5, depth_weight=0.2)


@dataclass
class SlamOptions:
    """Nobody has measured good defaults for the mapping side; these come from the only evidence in the tree.

    ``track``: ``gs_track.TrackOptions()`` as they are (the pose fit of tests/test_gpu_pose.py).  ``train``: the Trainer of
    tests/test_gpu_seed.py::_trainer -- ``n_iters_warmup=5, depth_weight=0.2`` -- whose 90 steps over three views are the only
    depth-supervised fit from seeds measured here (profiles/seed_rgbd.txt); ``map_iterations_first`` is that run's 30 steps
    per view.  ``seed``: ``gs_seed.DEFAULTS``.  ``map_iterations`` = 120 is a value fitted to ONE sequence, the eight-frame
    synthetic arc of tests/test_gpu_slam.py (windows of two and three views): with 30 and with 60 steps per keyframe the
    loop kept its pose errors within one frame's motion but left the first keyframe's colour loss above its seeded value,
    with 120 every keyframe ends below it (profiles/slam_sequence.txt).  ``overlap_min``, ``keyframe_every``, ``window`` and
    ``min_share`` have no evidence behind them yet.

    The learning-rate schedule: ``Slam`` numbers its mapping steps 0, 1, 2, ... over the WHOLE run and passes that count as
    ``i_iter``, so ``train.n_iters`` is the number of mapping steps over which the "exp" schedule takes the rates down to
    1 %, not the length of a fit to a fixed set of views.  A sequence has no known length; the default stays
    ``TrainOptions``' 7001, so that a run of a few hundred mapping steps trains at nearly the full rate (0.72 x after 500).
    Set it to the expected keyframes x ``map_iterations`` for a sequence that should anneal, or ``lr_decay="none"``.

    ``carry_optimizer`` and ``prune_every`` are off: with them off the loop issues exactly the calls it issued before they
    existed.  ``prune_opa_min`` = 0.005 and ``prune_scale_max`` = None (no scale test) have no evidence behind them: 0.005 is a
    quarter of the 0.02 the reference prunes below inside its own densification schedule (``gs_prune.DEFAULTS``); what the
    options did on the eight-frame arc is in profiles/slam_carry.txt."""
    track: TrackOptions = field(default_factory=TrackOptions)
    train: TrainOptions = field(default_factory=_map_train_options)
    seed: dict = field(default_factory=lambda: dict(gs_seed.DEFAULTS))
    stride: int = 2                 # lattice of the overlap count (the seed lattice is seed["stride"])
    near: Optional[float] = None    # a point counts for a keyframe beyond this camera z; None: the camera's `near`
    border: int = 0                 # pixels taken off each side of a keyframe's image in the overlap count
    overlap_min: float = 0.9        # keyframe when the last keyframe sees less than this share of the measured points ...
    keyframe_every: int = 5         # ... or this many frames have passed since it
    window: int = 4                 # views optimised together: the new keyframe + the window - 1 that share most with it
    min_share: float = 0.1          # ... among those that see at least this share of its measured points
    map_iterations_first: int = 30  # mapping steps on the first frame
    map_iterations: int = 120       # mapping steps per later keyframe, round-robin over the window (fitted: see above)
    max_pairs: int = 1 << 21        # the trainer's initial pair capacity (it grows by itself)
    # Joint refinement of the window's poses with the map (off: the loop is bit for bit the one without the option).  The
    # rates are TrackOptions' 2e-3 x 0.1, held constant: a window view takes some 30 - 60 pose steps per keyframe, which lets
    # it travel ~1e-2 (rad, scene units) at most and jitter by ~2e-4 -- an order below one frame's motion on the arc of
    # tests/test_gpu_pose_adam.py.  No evidence beyond that arc (profiles/pose_refine.txt).
    refine_poses: bool = False
    pose_lr_rot: float = 2e-4
    pose_lr_tran: float = 2e-4
    # Map edits that keep the optimizer state (off: the loop is call for call the one without the options)
    carry_optimizer: bool = False   # a keyframe's seeding keeps the old rows' Adam moments and the step count
    prune_every: int = 0            # prune behind the mapping steps of every k-th keyframe (0: never)
    prune_opa_min: float = 0.005    # ... the Gaussians with sigmoid(opa) <= this (no evidence: see above)
    prune_scale_max: Optional[float] = None  # ... or ||act(scale)|| >= this; None: no scale test
    # Visibility pruning (off: the loop issues exactly the calls it issues without the option): behind the mapping steps of
    # every k-th keyframe -- and behind prune_every's own prune -- the Gaussians that reach the weight prune_unseen_w_min at no
    # pixel of any keyframe are removed (Trainer.contributions over all keyframes, Trainer.prune(views_min=1)), the optimizer
    # state carried as carry_optimizer says.  1/255: below it no 8-bit colour channel moves by a whole level -- a reason for
    # the default and nothing more; what the option did on the eight-frame arc is in profiles/contrib_prune.txt.
    prune_unseen_every: int = 0
    prune_unseen_w_min: float = 1.0 / 255.0
    # Per-view exposure.  Tracking it arrives through ``track.fit_exposure``: a keyframe is then added to the trainer with its
    # tracked exposure, held fixed; keyframe 0 is the gauge -- the identity, no exposure object, never freed.  With
    # ``refine_exposure`` (off: the loop issues exactly the calls it issues without the option) the mapping steps of a keyframe
    # also step the exposures of its window (Trainer.free_exposure, on the device), every view but keyframe 0 -- the mirror
    # of ``refine_poses``.  The rates are TrackOptions' 3e-2 x 0.1, held constant, by the reasoning of ``pose_lr_rot``; no
    # evidence beyond the two-frame arc of tests/test_gpu_track_exposure.py (profiles/exposure.txt).
    refine_exposure: bool = False
    exposure_lr_gain: float = 3e-3
    exposure_lr_bias: float = 3e-3
    # Eviction of keyframes (0, the default: none -- no redundancy count is issued, the set grows to GS_OVERLAP_MAX_VIEWS and
    # the next keyframe raises, the loop issues exactly the calls it issues without the option).  3 .. 256: the most keyframes
    # held.  When a frame becomes a keyframe and the set holds that many, one keyframe goes first: for every keyframe the share
    # of its own measured points (lattice ``evict_stride``; None: ``stride``) that at least ``evict_seen_by`` OTHER keyframes see
    # is counted (KeyframeSet.redundancy: gs_view_redundancy per keyframe, one host read), and the one with the highest share
    # leaves the set and the trainer (select_eviction) -- never keyframe 0, the founder of the map and the gauge of
    # ``refine_poses``, never the last one, whose count the overlap rule reads.  The Gaussians it seeded stay.
    # ``evict_seen_by`` = 3 is ORB-SLAM's culling rule ("seen by at least three other keyframes"); nothing in this tree is
    # evidence for it.  What the option did on the eight-frame arc: profiles/evict.txt.
    max_keyframes: int = 0
    evict_seen_by: int = 3
    evict_stride: Optional[int] = None
    # The tracker's median gate carried into seeding and mapping (off: no GateMask and no extra renderer exist, the loop issues
    # exactly the calls it issues without the option).  Needs a gated tracker (``track.depth_gate_k`` or ``color_gate_k`` above
    # zero).  Every keyframe after the first renders the frozen map once at its tracked pose, turns the tracker's gate into a
    # range map without the rejected measurements and a 0 / 1 colour weight (gs_train.GateMask) and hands those to the trainer:
    # seeding and the depth loss see the gated range, the colour loss the weight.  The keyframe set keeps the raw range.  A
    # real new object in front of the map is rejected like an occluder while this is on.
    gate_map: bool = False
    # Depth alignment in front of the photometric tracker (None, the default: no aligner exists, no render is issued, the loop
    # is bit for bit the one without the option).  With ``gs_icp.IcpOptions``: every frame after the first renders the frozen
    # map's depth once at the pose the tracker would start from, aligns the frame's range map to it by point-to-plane ICP on
    # the device (gs_icp.IcpAligner: one host read) and, where the result is accepted, starts the tracker from it.  The
    # photometric iteration count stays ``track.iterations``.  What it did on the eight-frame arc: profiles/icp.txt.
    icp: Optional[IcpOptions] = None


@dataclass
class SlamFrame:
    rot: np.ndarray                  # [3,3] float64, world -> camera
    tran: np.ndarray                 # [3] float64
    tracked: Optional[TrackResult]   # None for the first frame
    keyframe: bool
    overlap: Optional[np.ndarray]    # counts [keyframes before this frame + 2]; None for the first frame
    window: List[int] = field(default_factory=list)   # keyframe indices optimised, the new one first
    added: int = 0                   # Gaussians seeded
    map_losses: List[float] = field(default_factory=list)  # the loss of each mapping step
    seconds: dict = field(default_factory=dict)  # wall time in track / overlap / seed / map (each ends on a host read)
    pending: int = 0                 # mapping steps that `Slam.map(frame)` has still to take (`begin` sets it)
    # refine_poses: keyframe index -> (rot, tran) float64 of every window view whose pose the mapping steps moved (never
    # keyframe 0); rot / tran above then report this frame's own refined pose
    refined: Dict[int, Tuple[np.ndarray, np.ndarray]] = field(default_factory=dict)
    pruned: int = 0                  # Gaussians removed behind this keyframe's mapping steps (prune_every)
    pruned_unseen: int = 0           # ... and those removed because no keyframe sees them (prune_unseen_every)
    # SlamOptions.max_keyframes: the stable id (KeyframeSet.ids) of the keyframe evicted to make room for this one, else None;
    # `window` holds positions AFTER that removal, `overlap` the counts as computed BEFORE it; seconds["evict"] its wall time
    evicted: Optional[int] = None
    window_ids: List[int] = field(default_factory=list)  # the stable ids of `window`
    # track.fit_exposure / refine_exposure: the frame's (gain [3], bias [3]) float64 -- as tracked, then as its mapping steps
    # left it; None with both off and for the first frame (the gauge: the identity)
    exposure: Optional[Tuple[np.ndarray, np.ndarray]] = None
    # SlamOptions.gate_map, a gated keyframe: (range pixels removed, pixels with colour weight 0); None otherwise
    gated: Optional[Tuple[int, int]] = None
    icp: Optional[IcpResult] = None  # SlamOptions.icp: the depth alignment in front of this frame's tracking, accepted or not


class Slam:
    """``Slam(camera, options)``: ``camera`` gives the image size, the focal lengths, ``near`` and the pose of the first
    frame.  ``step(image, range_map, init=None)`` takes one frame -- contiguous float32 HIP tensors [H,W,3] and [H,W]
    (range from the camera centre; <= 0, inf, NaN: no measurement) -- and returns a ``SlamFrame``.  ``init`` = (rot, tran):
    the first frame's pose, or where a later frame's tracking starts.  ``params`` is the map, ``keyframes`` the set.
    ``step`` is ``begin`` -- everything up to and including a keyframe's seeding -- followed by ``map`` -- its mapping steps
    and the tracker's rebind; a caller that wants to look at the map in between calls the two itself."""

    def __init__(self, camera, options: Optional[SlamOptions] = None, device="cuda"):
        self.opt = options if options is not None else SlamOptions()
        self.opt.track.fits_exposure()  # (refuses fit_exposure with device_pose before any device work)
        if self.opt.gate_map and not self.opt.track.gated():  # (before any device work)
            raise ValueError("SlamOptions.gate_map carries the tracker's median gate into seeding and mapping: it needs a gated "
                             "tracker (TrackOptions.depth_gate_k or color_gate_k above zero)")
        mk = int(self.opt.max_keyframes)
        if mk != 0 and not 3 <= mk <= GS_OVERLAP_MAX_VIEWS:  # (position 0 and the last one are never evicted)
            raise ValueError(f"SlamOptions.max_keyframes must be 0 (no eviction) or lie in [3, {GS_OVERLAP_MAX_VIEWS}]")
        if not 1 <= int(self.opt.evict_seen_by) <= GS_REDUNDANCY_BINS - 1:
            raise ValueError(f"SlamOptions.evict_seen_by must lie in [1, {GS_REDUNDANCY_BINS - 1}]")
        if self.opt.evict_stride is not None and int(self.opt.evict_stride) < 1:
            raise ValueError("SlamOptions.evict_stride must be None (the overlap count's stride) or >= 1")
        # the map is seeded with rgb colours; a `seed` dict that asks for SH rows is refused with the tracker's sentence
        self._seed = {k: v for k, v in self.opt.seed.items() if k != "color_dim"}
        if int(self.opt.seed.get("color_dim", 3)) != 3:
            raise RuntimeError(_SH_REFUSAL)
        self.device = require_hip(device, "Slam")
        self.camera = camera
        self.near = float(self.opt.near if self.opt.near is not None else camera.near)
        self.keyframes = KeyframeSet(device=self.device)
        self.trainer: Optional[Trainer] = None
        self.tracker: Optional[Tracker] = None
        self.aligner: Optional[IcpAligner] = None
        self.gate_mask: Optional[GateMask] = None
        self._gate_exposure = None  # gate_map with track.fit_exposure: compensates the render the gate is taken on
        self._icp_renderer = None
        if self.opt.icp is not None or self.opt.gate_map:
            # an inference renderer of their own, shared: the tracker's workspace and counters stay untouched
            from gs_frame import FrameRenderer

            self._icp_renderer = FrameRenderer(self.device, max_pairs=int(self.opt.track.max_pairs), training=False,
                                               occlusion_cull=False, auto_grow=True)
        if self.opt.icp is not None:
            self.aligner = IcpAligner(camera, self.opt.icp, self.device)
        if self.opt.gate_map:
            self.gate_mask = GateMask.from_track_options(int(camera.height), int(camera.width), self.opt.track, self.device)
        self.i_iter = 0          # mapping steps taken so far, over the whole run
        self.n_frames = 0
        self._last_keyframe_at = 0

    @property
    def params(self):
        return self.trainer.flat.params if self.trainer is not None else None

    def _posed(self, rot, tran):
        return posed(self.camera, rot, tran)

    def free_exposures(self, views: Sequence[int]):
        """Frees the exposures of the keyframes at positions ``views`` for the mapping steps that follow
        (``Trainer.free_exposure`` at ``exposure_lr_gain`` / ``exposure_lr_bias``).  Keyframe 0 is refused: it is the gauge --
        the map's radiometry is its radiometry -- and with it free a common gain could drift between map and exposures."""
        views = [int(v) for v in views]
        if 0 in views:
            raise ValueError("keyframe 0 fixes the radiometric gauge (the identity exposure): its exposure is never freed")
        for v in views:
            self.trainer.free_exposure(v, self.opt.exposure_lr_gain, self.opt.exposure_lr_bias)

    def map(self, frame: SlamFrame) -> SlamFrame:
        """The mapping steps of a keyframe that ``begin`` returned, round-robin over its window starting with the new view,
        then the tracker's (re)bind to the trainer's parameters.  A frame that is no keyframe has none: nothing happens."""
        if not frame.keyframe:
            return frame
        t0 = time.perf_counter()
        o, tr = self.opt, self.trainer
        # refine_poses: every view of the window but keyframe 0 (the gauge) is free for these steps
        freed = [v for v in frame.window if v != 0] if (o.refine_poses and frame.pending > 0) else []
        before = {v: (tr.cameras[v].rot, tr.cameras[v].tran) for v in freed}
        for v in freed:
            tr.free_pose(v, o.pose_lr_rot, o.pose_lr_tran)
        # refine_exposure: likewise, on the device
        freed_ex = [v for v in frame.window if v != 0] if (o.refine_exposure and frame.pending > 0) else []
        self.free_exposures(freed_ex)
        vals = []
        for s in range(frame.pending):
            vals.append(self.trainer.train_step(self.i_iter, frame.window[s % len(frame.window)]).clone())
            self.i_iter += 1
        frame.pending = 0
        for v in freed_ex:
            tr.fix_exposure(v)
        if freed_ex and frame.window[0] in freed_ex:
            frame.exposure = tr.exposure(frame.window[0])  # (one host read)
            if frame.tracked is not None and self.tracker is not None and self.opt.track.fit_exposure:
                self.tracker.set_last_exposure(*frame.exposure)  # the next frame's exposure fit starts from the refined one
        for v in freed:
            rot, tran = tr.pose(v)  # (float64; settles the last step's update)
            tr.fix_pose(v)
            cam = tr.cameras[v]
            if not (np.array_equal(cam.rot, before[v][0]) and np.array_equal(cam.tran, before[v][1])):
                self.keyframes.set_pose(v, cam.rot, cam.tran)  # the float32 pose the trainer renders: the two agree
                frame.refined[v] = (rot, tran)
        if frame.window and frame.window[0] in frame.refined:
            frame.rot, frame.tran = frame.refined[frame.window[0]]
            if frame.tracked is not None:  # the next frame's constant-velocity prediction starts from the refined pose
                self.tracker.set_last_pose(frame.rot, frame.tran)
        frame.map_losses += [float(v) for v in torch.stack(vals)[:, 0].cpu()] if vals else []
        frame.seconds["map"] = time.perf_counter() - t0
        # (every k-th keyframe ADDED: with eviction the set's length stops growing, the number of keyframes taken does not)
        if o.prune_every > 0 and self.keyframes.n_added % int(o.prune_every) == 0:
            t0 = time.perf_counter()
            frame.pruned = tr.prune(self.i_iter, opa_min=o.prune_opa_min, scale_max=o.prune_scale_max,
                                    carry_state=bool(o.carry_optimizer))
            frame.seconds["prune"] = time.perf_counter() - t0
        if o.prune_unseen_every > 0 and self.keyframes.n_added % int(o.prune_unseen_every) == 0:
            # what reaches w_min in no keyframe is constrained by no training view: seeds that ended up behind a surface,
            # duplicates from several keyframes, whatever lies outside every frustum
            t0 = time.perf_counter()
            seen = tr.contributions(w_min=o.prune_unseen_w_min)
            frame.pruned_unseen = tr.prune(self.i_iter, contributions=seen, views_min=1, carry_state=bool(o.carry_optimizer))
            frame.seconds["prune_unseen"] = time.perf_counter() - t0
        # (also with no step taken: seeding gave the trainer new parameter tensors)
        if self.tracker is None:
            self.tracker = Tracker(self.trainer.flat.params, self.keyframes.cameras[0], self.opt.track, self.device)
        else:
            self.tracker.set_map(self.trainer.flat.params)
        return frame

    def _align(self, range_map, init) -> IcpResult:
        """The depth alignment of ``SlamOptions.icp``: the frozen map's depth and alpha rendered once at the pose the tracker
        would start from (its constant-velocity prediction, or ``init``), the frame's range map aligned to them.  The map's
        tensors are read, never written."""
        cam = self._posed(*self.tracker._start_pose(init))
        _, _, depth, alpha = self._icp_renderer.forward(*self.tracker.params, cam, training=False, aux=True)
        # (the model view is the float32 pose that was rendered; the frame starts from the same pose: the identity)
        self.aligner.set_model(depth.contiguous(), alpha.contiguous(), cam.rot.astype(np.float64), cam.tran.astype(np.float64))
        return self.aligner.align(range_map)

    def _first(self, image, range_map, init) -> SlamFrame:
        o = self.opt
        rot, tran = init if init is not None else (self.camera.rot, self.camera.tran)
        rot, tran = pose64(rot, tran)
        cam = self._posed(rot, tran)
        t0 = time.perf_counter()
        params = gs_seed.seed_from_depth(image, range_map, cam, color_dim=3, **self._seed)
        if int(params[0].shape[0]) == 0:
            raise RuntimeError("the first frame carries no measurement: nothing to found the map on")
        self.trainer = Trainer(params, [cam], [image], o.train, max_pairs=int(o.max_pairs), depths=[range_map])
        frame = SlamFrame(rot=rot, tran=tran, tracked=None, keyframe=True, overlap=None, window=[0],
                          added=int(params[0].shape[0]), pending=int(o.map_iterations_first))
        frame.window_ids = [self.keyframes.ids[self.keyframes.add(cam, image, range_map)]]
        frame.seconds["seed"] = time.perf_counter() - t0
        return frame

    def step(self, image: torch.Tensor, range_map: torch.Tensor, init=None) -> SlamFrame:
        return self.map(self.begin(image, range_map, init))

    def begin(self, image: torch.Tensor, range_map: torch.Tensor, init=None) -> SlamFrame:
        """Track, count, decide and -- for a keyframe -- add the view and seed its Gaussians.  ``map(frame)`` must follow
        before the next frame."""
        o = self.opt
        if self.trainer is None:
            frame = self._first(image, range_map, init)
            self.n_frames, self._last_keyframe_at = 1, 0
            return frame
        icp = None
        if self.aligner is not None:
            ti = time.perf_counter()
            icp = self._align(range_map, init)
            if icp.accepted:
                init = (icp.rot, icp.tran)
            ti = time.perf_counter() - ti
        t0 = time.perf_counter()
        res = self.tracker.track(image, range_map, init)
        t1 = time.perf_counter()
        cam = self._posed(res.rot, res.tran)
        n = len(self.keyframes)
        counts = self.keyframes.overlap(range_map, cam, stride=o.stride, near=self.near, border=o.border)
        t2 = time.perf_counter()
        measured = int(counts[n])
        frames_since = self.n_frames - self._last_keyframe_at
        frame = SlamFrame(rot=res.rot, tran=res.tran, tracked=res, overlap=counts,
                          keyframe=is_keyframe(int(counts[n - 1]), measured, frames_since, o.overlap_min, o.keyframe_every))
        frame.seconds.update(track=t1 - t0, overlap=t2 - t1)
        frame.exposure = res.exposure  # (None without track.fit_exposure)
        if icp is not None:
            frame.icp = icp
            frame.seconds["icp"] = ti
        evict = frame.keyframe and n >= int(o.max_keyframes) > 0
        if frame.keyframe and n >= self.keyframes.capacity and not evict:  # before the trainer or the frame count is touched
            raise RuntimeError(f"the keyframe set is full ({self.keyframes.capacity} views); there is no eviction")
        index = self.n_frames
        self.n_frames += 1
        if not frame.keyframe:
            return frame
        window_counts = counts[:n]
        if evict:
            # the set is at its cap: the keyframe whose measured points the others see best goes first -- never position 0 (the
            # founder of the map, the gauge of refine_poses) and never the last (the overlap rule reads its count).  One host read.
            te = time.perf_counter()
            hists = self.keyframes.redundancy(stride=int(o.evict_stride if o.evict_stride is not None else o.stride),
                                              near=self.near, border=o.border)
            gone = select_eviction(hists, o.evict_seen_by, protected=(0, n - 1))
            if gone is None:
                raise RuntimeError(f"no keyframe of {n} can be evicted")
            frame.evicted = self.keyframes.ids[gone]
            self.keyframes.remove(gone)
            self.trainer.remove_view(gone)
            if len(self.trainer.cameras) != len(self.keyframes):
                raise RuntimeError(f"{len(self.keyframes)} keyframes against {len(self.trainer.cameras)} views of the trainer: "
                                   "the two lists have diverged")
            window_counts = np.delete(window_counts, gone)
            n -= 1
            frame.seconds["evict"] = time.perf_counter() - te
            t2 += frame.seconds["evict"]  # (seconds["seed"] below stays the time of adding and seeding)
        map_range, map_weight = range_map, None
        if self.gate_mask is not None:
            # the frozen map once more, at the tracked pose, with its aux maps; the tracker's gate on it gives what the
            # trainer sees of this keyframe (clones: the GateMask's maps are rewritten by the next keyframe).  One host read.
            tg = time.perf_counter()
            rimg, _, rdepth, ralpha = self._icp_renderer.forward(*self.tracker.params, cam, training=False, aux=True)
            rimg = rimg.contiguous()
            if res.exposure is not None:  # the tracker's gate was taken on the compensated render: so is this one
                if self._gate_exposure is None:
                    from gs_exposure import Exposure

                    self._gate_exposure = Exposure(self.gate_mask.H, self.gate_mask.W, self.device)
                self._gate_exposure.set(*res.exposure)
                rimg = self._gate_exposure.apply(rimg)
            g_range, g_weight = self.gate_mask(rimg, rdepth.contiguous(), ralpha.contiguous(), image, range_map)
            map_range, map_weight = g_range.clone(), g_weight.clone()
            v = self.gate_mask.values.tolist()
            frame.gated = (int(v[2]), int(self.gate_mask.H * self.gate_mask.W - v[3]))
            frame.seconds["gate"] = time.perf_counter() - tg
        new = self.keyframes.add(cam, image, range_map)  # (the raw range: the overlap count reads what was measured)
        added_as = self.trainer.add_view(cam, image, map_range, weight=map_weight, exposure=res.exposure)
        if added_as != new:
            raise RuntimeError(f"keyframe {new} became view {added_as} of the trainer: the two lists have diverged")
        self._last_keyframe_at = index
        frame.added = self.trainer.seed_from_view(new, self.i_iter, carry_state=bool(o.carry_optimizer), **self._seed)
        frame.seconds["seed"] = time.perf_counter() - t2
        frame.window = [new] + select_keyframes(window_counts, measured, o.window - 1, o.min_share)
        frame.window_ids = [self.keyframes.ids[v] for v in frame.window]
        frame.pending = int(o.map_iterations)
        return frame
