"""Camera tracking against a frozen map: the pose of an incoming RGB(-D) frame by rendering the map and descending on the
pose alone -- what an RGB-D pipeline does once per frame, before any mapping.

One iteration, without autograd:

    posed camera (host, by value) -> forward(training=True, aux=True) -> gs_loss_track (gs_train.TrackLoss)
      -> backward(part=GS_BWD_RASTER) -> backward(part=GS_BWD_GEOMETRY, grad_pose=...) -> one 64-byte read -> SE(3) step

With ``TrackOptions.depth_gate_k`` or ``color_gate_k`` above zero the loss is gs_loss_track_gated (gs_train.GatedTrackLoss): a
term counts where its residual is at most k x the frame's own median residual, selected on the device every iteration; the
buffer then holds 20 floats and the read 80 bytes -- still one read per iteration.

With ``TrackOptions.pose_only`` the two backward calls are one ``backward_pose(part=0)`` (gs_frame_backward_pose): the raster
backward, then ONE kernel that sums every Gaussian's rows and forms its pose terms -- the depth map's as well -- and the
reduction.  The same pose gradient bit for bit, so the same track; no projection or activation backward runs, no
per-Gaussian gradient is stored and the Tracker allocates no per-Gaussian scratch.  Off by default.

The colour part of the backward (GS_BWD_COLOR: opacity and colour gradients) is never run: nobody reads it.  dL/drot,
dL/dtran and the four loss values are views of one 16-float device buffer that a single copy brings into pinned host memory.
The pose step runs on the host in float64: rot = exp([w]x) R re-linearised at w = 0 every iteration, Adam on (w, tran),
R <- exp([dw]x) R -- rot stays on SO(3) by construction.  The map's parameters are never written.

With ``TrackOptions.device_pose`` the pose itself lives on the device: every frame is a GS_FRAME_DEVICE_POSE frame that reads
its 12 floats from ``pose_dev``, and one gs_pose_step launch behind ``backward_pose`` takes the Adam step there (PoseAdam,
so3_exp, rot_tangent_grad and the best-pose bookkeeping below, restated in double in pose_step.hip) and logs the iteration.
A whole ``track`` call is enqueued without a host wait and read back ONCE; a frame that overflowed its workspace is skipped
on the device and the call run again in a larger one.  Implies ``pose_only``.  Off by default.

Coarse to fine: ``TrackOptions.pyramid`` = ((level, iterations), ...) walks pyramid levels in order (gs_pyramid: the targets of
level l are gs_pyramid_down applied l times, its camera the frame's with size, focal lengths and principal point / 2^l), one
renderer and one loss object per scheduled level, ONE PoseAdam for the whole call.  With the default () nothing of this exists
and every call is the call described above.

With ``TrackOptions.fit_exposure`` the frame's affine exposure (gs_exposure.Exposure: gain[3] and bias[3] in device memory) is
fitted with the pose: forward -> gs_exposure_apply -> the loss on the compensated render, TrackLoss or GatedTrackLoss unchanged
-> gs_exposure_backward (the colour gradient map scaled in place, the six gradients, one Adam step on the six numbers on the
device at the iteration's decay) -> the pose backward as before.  One exposure fit per call, shared by the levels; the read
grows by 24 bytes; ``TrackResult.exposure`` is the exposure the returned pose's iteration rendered with.  Refused with
``device_pose``.  Off by default: the Tracker then issues the calls it always issued.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

from gaussian import _lib
from gs_call import check_tensor, require_hip
from gs_frame import FrameRenderer
from gs_geometry import pose64, posed
from gs_pyramid import MAX_LEVELS, Pyramid, level_camera
from gs_train import GatedTrackLoss, TrackLoss


@dataclass
class TrackOptions:
    """Defaults: the pose fit of tests/test_gpu_pose.py::test_pose_recovery (Adam, lr 2e-3 for both groups decaying to 0.01 x
    over 300 iterations, the silhouette at alpha 0.5, mean |I - T| per colour element + mean |r| per pixel)."""
    iterations: int = 300
    lr_rot: float = 2e-3
    lr_tran: float = 2e-3
    lr_final: float = 0.01          # the learning rates decay exponentially to this factor over the run
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    alpha_min: float = 0.5          # a pixel counts where the map's alpha reaches this
    color_weight: float = 1.0 / 3.0  # x sum_c |I_c - T_c| / (H W): the mean over the colour elements
    depth_weight: float = 1.0       # x |D / A - z| / (H W)
    depth_gate: float = 0.0         # <= 0: off; else depth residuals beyond it do not count
    max_pairs: int = 1 << 20        # the renderer's initial pair capacity (it grows by itself)
    # the pose gradient through FrameRenderer.backward_pose: no per-Gaussian gradient is computed or stored (bit for bit the
    # same pose gradient, so the same track)
    pose_only: bool = False
    # the pose in device memory, stepped there by gs_pose_step: no host wait inside ``track``, one read at its end (implies
    # pose_only; the renderers do not grow by themselves: an overflowed call is run again, ``TrackResult.attempts``)
    device_pose: bool = False
    # the frame's affine exposure (gs_exposure.Exposure: gain[3], bias[3]) fitted with the pose: the colour loss is taken on the
    # compensated render and every iteration takes one Adam step on the six numbers on the device, at the iteration's decay
    # and with ``betas`` / ``eps`` above; the iteration's read grows by 24 bytes.  Not with ``device_pose``.  The rates are
    # those of the exposure-only fit of tests/test_gpu_track_exposure.py, the only evidence there is
    fit_exposure: bool = False
    lr_gain: float = 3e-2
    lr_bias: float = 3e-2
    # coarse to fine: stages (pyramid level, iterations) in order, levels strictly decreasing; () (the default): no pyramid,
    # ``iterations`` full-resolution iterations.  With a schedule ``iterations`` is not read: the total is the stages' sum
    pyramid: Tuple[Tuple[int, int], ...] = ()
    # the median gate (gs_loss_track_gated): a k <= 0 leaves that term ungated; both <= 0 (the default) is gs_loss_track
    depth_gate_k: float = 0.0       # depth counts where |r| <= max(k x median |r|, depth_gate_floor); excludes depth_gate
    color_gate_k: float = 0.0       # colour counts where sum_c |I_c - T_c| <= max(k x its median, color_gate_floor)
    depth_gate_floor: float = 0.0
    color_gate_floor: float = 0.0
    gate_couple: bool = True        # a pixel that fails the depth gate loses its colour term too

    def fits_exposure(self) -> bool:
        """Whether the exposure is fitted; refuses the option together with ``device_pose``."""
        if self.fit_exposure and self.device_pose:
            raise ValueError("fit_exposure is not available with device_pose: gs_pose_step's log row has no room for the six "
                             "numbers and the best-pose bookkeeping lives there; track with the pose on the host")
        return bool(self.fit_exposure)

    def gated(self) -> bool:
        """Whether the median gate is on (-> GatedTrackLoss and the 20-float buffer); refuses the two depth gates together."""
        if self.depth_gate > 0.0 and self.depth_gate_k > 0.0:
            raise ValueError("depth_gate (a fixed threshold) and depth_gate_k (a multiple of the median residual) both gate "
                             "the depth term: give one of them")
        return self.depth_gate_k > 0.0 or self.color_gate_k > 0.0

    def stages(self) -> Tuple[Tuple[int, int], ...]:
        """``pyramid`` validated, as a tuple of (level, iterations) ints: levels within 0..GS_PYRAMID_MAX_LEVELS and strictly
        decreasing, iterations >= 1.  () for no schedule."""
        out = []
        for stage in self.pyramid:
            if len(stage) != 2 or any(int(x) != x for x in stage):
                raise ValueError(f"pyramid holds pairs (level, iterations) of integers, got {stage!r}")
            level, n = int(stage[0]), int(stage[1])
            if not 0 <= level <= MAX_LEVELS:
                raise ValueError(f"pyramid level {level} is outside 0..{MAX_LEVELS} (GS_PYRAMID_MAX_LEVELS)")
            if out and level >= out[-1][0]:
                raise ValueError(f"pyramid levels must be strictly decreasing (coarse to fine): {level} follows {out[-1][0]}")
            if n < 1:
                raise ValueError(f"pyramid level {level} is scheduled for {n} iterations: at least 1")
            out.append((level, n))
        return tuple(out)


@dataclass
class TrackResult:
    rot: np.ndarray      # [3,3] float64, world -> camera, on SO(3)
    tran: np.ndarray     # [3] float64
    loss: float          # the lowest loss seen: the loss of (rot, tran)
    iterations: int
    losses: List[float] = field(default_factory=list)  # per iteration, the loss of the pose that iteration rendered
    # With the median gate on, from the iteration that rendered (rot, tran) -- plain attributes, None with the gate off:
    inliers = None       # (depth pixels that counted, n_d = covered measured pixels, colour pixels that counted)
    medians = None       # (m_d, m_c): the median residuals the thresholds were multiples of
    # With a schedule (TrackOptions.pyramid): [(level, index of its first iteration in ``losses``, count), ...]; else None
    levels = None
    log = None           # TrackOptions.device_pose: float32 [iterations, 24 + n] -- per row the 12 pose floats the iteration
    #                      rendered, dL/drot [9], dL/dtran [3] and the loss's n values; else None
    attempts = 1         # runs of the call (TrackOptions.device_pose: one more per workspace growth; else always 1)
    exposure = None      # TrackOptions.fit_exposure: (gain [3], bias [3]) float64 that (rot, tran)'s iteration rendered with


def so3_exp(w) -> np.ndarray:
    """exp([w]x) in float64 (Rodrigues; the series below 1e-8 rad)."""
    w = np.asarray(w, np.float64).reshape(3)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def rot_tangent_grad(grad_rot, rot) -> np.ndarray:
    """dL/dw at w = 0 of rot(w) = exp([w]x) rot, from G = dL/drot: with M = G rot^T, (M32 - M23, M13 - M31, M21 - M12)."""
    M = np.asarray(grad_rot, np.float64).reshape(3, 3) @ np.asarray(rot, np.float64).reshape(3, 3).T
    return np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])


def predict_constant_velocity(prev, last):
    """T_pred = T_last T_prev^-1 T_last in float64 for world -> camera poses (rot, tran): the motion between the last two
    frames, applied once more."""
    (Rp, tp), (Rl, tl) = pose64(*prev), pose64(*last)
    dR = Rl @ Rp.T               # T_last T_prev^-1 = (dR, tl - dR tp)
    dt = tl - dR @ tp
    R = dR @ Rl
    U, _, Vt = np.linalg.svd(R)  # (two products of rotations: back onto SO(3) to the last bit)
    return U @ Vt, dR @ tl + dt


_SH_REFUSAL = ("pose gradients need rgb colours: with SH colours the image also depends on the pose through "
               "each pixel's ray direction, which the backward does not differentiate")


class PoseAdam:
    """The pose optimizer, stated once (Tracker.track, gs_train.Trainer's free poses): a world -> camera pose (rot on SO(3),
    tran) in float64 on the host and Adam on its six tangent numbers.  One ``step``: g = (dL/dw at w = 0 of rot(w) =
    exp([w]x) rot, dL/dtran), Adam's moments and bias corrections on g, then rot <- exp([-dw]x) rot, tran <- tran - dt --
    rot stays on SO(3) by construction.  ``k`` counts the steps taken."""

    def __init__(self, rot, tran, lr_rot: float, lr_tran: float, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8):
        self.rot, self.tran = pose64(rot, tran)
        self.lr0 = np.array([lr_rot] * 3 + [lr_tran] * 3)
        self.betas = (betas[0], betas[1])
        self.eps = eps
        self.m, self.v = np.zeros(6), np.zeros(6)
        self.k = 0

    def step(self, grad_rot, grad_tran, lr_scale: float = 1.0):
        """``grad_rot`` [9] / [3,3] = dL/drot, ``grad_tran`` [3] = dL/dtran (float64); ``lr_scale`` multiplies both learning
        rates for this step.  Returns the new (rot, tran)."""
        b1, b2 = self.betas
        g = np.concatenate([rot_tangent_grad(grad_rot, self.rot), np.asarray(grad_tran, np.float64).reshape(3)])
        self.k += 1
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        step = self.lr0 * lr_scale * (self.m / (1.0 - b1 ** self.k)) / (np.sqrt(self.v / (1.0 - b2 ** self.k)) + self.eps)
        self.rot = so3_exp(-step[:3]) @ self.rot
        self.tran = self.tran - step[3:]
        return self.rot, self.tran


class FreePose:
    """A pose that a training loop refines without waiting for its gradient (gs_train.Trainer.free_pose): the step's backward
    writes dL/drot, dL/dtran into ``grad_pose`` (views of ``dev``), ``deliver`` sends the 48 bytes to pinned host memory behind
    it, and ``settle`` -- called by whoever reads the pose next -- waits for that copy and takes the ``PoseAdam`` step.  As
    long as every reader settles first, that is exactly the step taken at once.  Without a device (``device=None``) the
    gradient is written into ``host`` directly: the same bookkeeping on the host alone."""

    def __init__(self, adam: PoseAdam, device=None):
        self.adam = adam
        self.pending = False
        self.host = torch.zeros(12, dtype=torch.float32)  # grad_rot [0:9], grad_tran [9:12]
        self.dev = self.grad_pose = self.event = None
        if device is not None:
            self.host = self.host.pin_memory()
            self.dev = torch.zeros(12, dtype=torch.float32, device=device)
            self.grad_pose = (self.dev[0:9].view(3, 3), self.dev[9:12])
            self.event = torch.cuda.Event()

    def deliver(self):
        """Behind the step that wrote the gradient, on the stream that ran it: no host synchronisation."""
        if self.dev is not None:
            self.host.copy_(self.dev, non_blocking=True)
            self.event.record()
        self.pending = True

    def settle(self) -> bool:
        """Take the pending step, if any -> whether the pose moved (was stepped)."""
        if not self.pending:
            return False
        self.pending = False
        if self.event is not None:
            self.event.synchronize()
        h = self.host.numpy().astype(np.float64)
        self.adam.step(h[0:9], h[9:12])
        return True


class Tracker:
    """``Tracker(params, camera)``: ``params`` = (pos, quat, scale, opa, rgb) of an rgb map, ``camera`` gives the image size,
    the focal lengths, ``near`` and the pose tracking starts from.  ``track(image, range_map)`` estimates the pose of one
    incoming frame; without ``init`` it starts from the constant-velocity prediction of the last two tracked poses, else
    the last pose, else the camera's."""

    def __init__(self, params, camera, options: Optional[TrackOptions] = None, device="cuda"):
        self.opt = options if options is not None else TrackOptions()
        if self.opt.device_pose and not self.opt.pose_only:  # (the only backward a device-pose frame has)
            self.opt = replace(self.opt, pose_only=True)
        fit_exposure = self.opt.fits_exposure()  # (refused with device_pose before any device work)
        self._check_map(params)
        self.device = require_hip(device, "Tracker")
        self.camera = camera
        self.H, self.W = int(camera.height), int(camera.width)
        plan = self.level_plan(self.opt, self.H, self.W)
        self.renderer = self._new_renderer()
        self.device = self.renderer.device
        cls, args, nfloat = self.loss_plan(self.opt, self.H, self.W)
        # grad_rot [0:9], grad_tran [9:12], (loss, colour term, depth term, depth pixels) [12:16] and, with the median gate,
        # (colour pixels, m_d, m_c, n_d) [16:20]: one read per iteration.  fit_exposure: six floats more behind them, the
        # exposure's own numbers (gs_exposure.Exposure adopts them: the read brings what the iteration's step left, which is
        # what the next iteration renders with -- the first one's are known to the host)
        self._nfloat = nfloat
        self._dev = torch.zeros(nfloat + (6 if fit_exposure else 0), dtype=torch.float32, device=self.device)
        self._grad_pose = (self._dev[0:9].view(3, 3), self._dev[9:12])
        self._values = self._dev[12:nfloat]
        self._host = torch.zeros(self._dev.numel(), dtype=torch.float32).pin_memory()
        # per level an Exposure with buffers of its own, all on the same six numbers and the same Adam state; None: option off
        self._exposures = None
        if fit_exposure:
            from gs_exposure import Exposure

            sizes = [(0, self.H, self.W)] if plan is None else plan
            first = Exposure(sizes[0][1], sizes[0][2], self.device, numbers=self._dev[nfloat:nfloat + 6])
            self._exposures = {sizes[0][0]: first}
            for level, h, w in sizes[1:]:
                self._exposures[level] = first.sibling(h, w)
        if plan is None:  # no schedule: one renderer, one loss, no Pyramid
            self.loss = cls(*args, self.device)
            self._stages = self._levels = self._pyramid = None
        else:
            # per scheduled level (renderer, loss, camera, scale): a renderer and a loss object of its own, the level camera,
            # scale = 1 / (H_l W_l) so that every level's loss is a mean; the two buffers above are shared
            self._stages = self.opt.stages()
            self._levels = {}
            for level, h, w in plan:
                r = self.renderer if not self._levels else self._new_renderer()
                lcls, largs, _ = self.loss_plan(self.opt, h, w)
                self._levels[level] = (r, lcls(*largs, self.device), level_camera(camera, level), 1.0 / (h * w))
            self.renderer, self.loss = self._levels[plan[-1][0]][:2]  # the finest scheduled level's
            self._pyramid = Pyramid(self.H, self.W, plan[0][0], self.device)
        self._scratch = None
        self._dp = None  # TrackOptions.device_pose: the device state + log, pose_dev and their pinned host copy (_device_buffers)
        if self.opt.device_pose:
            self._device_buffers(sum(n for _, n in self._stages) if self._stages else int(self.opt.iterations), nfloat - 12)
        self.set_map(params)
        self.reset()

    @staticmethod
    def loss_plan(o: TrackOptions, height: int, width: int):
        """(loss class, its arguments before the device, floats per iteration) for these options -- no device needed.  Gate
        off: TrackLoss and 16 floats, exactly the calls of a tracker without the gate; on: GatedTrackLoss and 20."""
        if not o.gated():
            return TrackLoss, (height, width, o.alpha_min, o.color_weight, o.depth_weight, o.depth_gate), 16
        return GatedTrackLoss, (height, width, o.alpha_min, o.color_weight, o.depth_weight, o.depth_gate_k, o.color_gate_k,
                                o.depth_gate_floor, o.color_gate_floor, o.gate_couple), 20

    @staticmethod
    def level_plan(o: TrackOptions, height: int, width: int):
        """[(level, H_l, W_l)] of the stages of ``o.pyramid`` in order, None without a schedule -- no device needed.  Refuses
        what ``TrackOptions.stages`` refuses and a frame size the deepest scheduled level does not divide."""
        stages = o.stages()
        if not stages:
            return None
        deepest = stages[0][0]
        if height % (1 << deepest) or width % (1 << deepest):
            raise ValueError(f"a {width} x {height} frame cannot be tracked at pyramid level {deepest}: 2^{deepest} = "
                             f"{1 << deepest} does not divide its size")
        return [(level, height >> level, width >> level) for level, _ in stages]

    def _new_renderer(self):
        # (device_pose: reading the pair counters after every frame is one of the two waits the option removes)
        return FrameRenderer(self.device, max_pairs=int(self.opt.max_pairs), training=True, occlusion_cull=False,
                             auto_grow=not self.opt.device_pose)

    @staticmethod
    def _check_map(params):
        if len(params) != 5:
            raise ValueError("params must be (pos, quat, scale, opa, rgb)")
        rgb = params[4]
        if rgb.dim() != 2 or rgb.shape[1] != 3:
            raise RuntimeError(_SH_REFUSAL)

    def set_map(self, params):
        """Rebind the map (after the mapper changed or grew the Gaussian set).  The tensors are read, never written."""
        self._check_map(params)
        for name, t in zip(("pos", "quat", "scale", "opa", "rgb"), params):
            check_tensor(name, t)
        self.params = tuple(t.detach() for t in params)
        if self.opt.pose_only:
            return  # (backward_pose has no per-Gaussian destination)
        if self._scratch is None or any(s.shape != p.shape for s, p in zip(self._scratch, self.params)):
            # the per-Gaussian gradient rows the backward writes on its way to the pose gradient: nobody reads them
            self._scratch = tuple(torch.empty_like(p) for p in self.params)

    def reset(self):
        """Forget the motion history: the next ``track`` without ``init`` starts from the constructor camera's pose."""
        self._history: List[Tuple[np.ndarray, np.ndarray]] = []
        self._last_exposure = None  # fit_exposure: the six float32 numbers of the last tracked frame

    def set_last_pose(self, rot, tran):
        """Replace the last tracked pose of the motion history (a mapper refined the pose of the frame just tracked): the
        constant-velocity prediction of the next ``track`` starts from it."""
        if not self._history:
            raise RuntimeError("set_last_pose() needs a tracked frame")
        self._history[-1] = pose64(rot, tran)

    def set_last_exposure(self, gain, bias):
        """Replace the last tracked frame's exposure (a mapper refined it): the exposure fit of the next ``track`` starts from
        it.  ``TrackOptions.fit_exposure`` only."""
        if self._exposures is None:
            raise RuntimeError("set_last_exposure() needs TrackOptions.fit_exposure")
        from gs_exposure import numbers32

        self._last_exposure = numbers32(gain, bias)

    def _start_pose(self, init):
        if init is not None:
            return pose64(*init)
        if len(self._history) >= 2:
            return predict_constant_velocity(self._history[-2], self._history[-1])
        if self._history:
            return pose64(*self._history[-1])
        return pose64(self.camera.rot, self.camera.tran)

    def iteration(self, rot, tran, image, range_map=None, level=0, lr_scale=1.0):
        """One forward / loss / pose backward at the pose (rot, tran); the 16 floats land in ``self._host`` (pinned):
        dL/drot [0:9], dL/dtran [9:12], (loss, colour term, depth term, depth pixels) [12:16]; with the median gate 20 floats,
        [16:20] = (colour pixels, m_d, m_c, n_d).  Returns that buffer.  ``level``: a scheduled level of ``TrackOptions.pyramid``
        -- ``image`` / ``range_map`` are then that level's targets (gs_pyramid.Pyramid.build), rendered through the level camera;
        without a schedule only level 0 exists.  ``TrackOptions.fit_exposure``: the loss is taken on the compensated render,
        the exposure's backward scales the colour gradient map and -- inside ``track``, where the exposure is free -- steps the
        six numbers at ``lr_scale`` x their rates; the buffer ends with six floats more, the numbers AFTER that step."""
        if self._levels is None:
            if level != 0:
                raise ValueError(f"level {level}: this Tracker has no schedule (TrackOptions.pyramid), only level 0")
            r, loss, camera, scale = self.renderer, self.loss, self.camera, 1.0 / (self.H * self.W)
        elif level in self._levels:
            r, loss, camera, scale = self._levels[level]
        else:
            raise ValueError(f"level {level} is not in this Tracker's schedule {self._stages}")
        cam = posed(camera, rot, tran)
        img, _, depth, alpha = r.forward(*self.params, cam, training=True, aux=True)
        with torch.cuda.device(self.device):
            if self._exposures is None:
                gi, gd, ga = loss(img, depth, alpha, image, range_map, scale, values=self._values)
            else:
                ex = self._exposures[level]
                gi, gd, ga = loss(ex.apply(img), depth, alpha, image, range_map, scale, values=self._values)
                ex.backward(img, gi, lr_scale)
        if self.opt.pose_only:
            r.backward_pose(gi, self._grad_pose, 0, grad_depth=gd, grad_alpha=ga)
        else:
            r.backward(gi, out=self._scratch, part=_lib.GS_BWD_RASTER, grad_depth=gd, grad_alpha=ga)
            r.backward(None, out=self._scratch, part=_lib.GS_BWD_GEOMETRY, grad_pose=self._grad_pose)
        self._host.copy_(self._dev)  # (device -> pinned host: returns when the 64 -- gated: 80 -- bytes have landed)
        return self._host

    def track(self, image, range_map=None, init=None, init_exposure=None) -> TrackResult:
        """``image`` [H,W,3] and ``range_map`` [H,W] (range from the camera centre; <= 0, inf, NaN: no measurement; None:
        RGB only): contiguous float32 tensors on the tracker's device.  Returns the pose with the lowest loss seen.
        ``init_exposure`` = (gain, bias) (``TrackOptions.fit_exposure`` only): where the exposure fit starts; without it from
        the last tracked frame's exposure, else from the identity."""
        o = self.opt
        if init_exposure is not None and self._exposures is None:
            raise ValueError("init_exposure needs TrackOptions.fit_exposure")
        R, t = self._start_pose(init)
        if o.device_pose:
            return self._track_on_device(R, t, image, range_map)
        adam = PoseAdam(R, t, o.lr_rot, o.lr_tran, o.betas, o.eps)  # Adam's moments on (w, tran): kept across iterations, reset per call
        nf, ex32 = self._nfloat, None
        if self._exposures is not None:
            # ONE exposure fit for the call: the numbers start over, Adam's state on the device from zero (shared by the levels)
            from gs_exposure import numbers32

            ex32 = numbers32(*init_exposure) if init_exposure is not None else \
                self._last_exposure if self._last_exposure is not None else numbers32()
            ex = next(iter(self._exposures.values()))
            ex.set(ex32[0:3], ex32[3:6])
            ex.free(o.lr_gain, o.lr_bias, o.betas, o.eps)
        best = (math.inf, R, t, None, ex32)
        losses: List[float] = []
        # coarse to fine: the targets once, then the stages in order under ONE PoseAdam (moments and step count carry across
        # stages, the rate decays over the whole call); losses of different levels are not comparable, so the pose returned
        # is the lowest-loss one of the LAST stage.  Without a schedule: one stage at level 0 on the caller's tensors
        stages, images, ranges, total = self._stage_list(image, range_map)
        levels, k = [], 0
        for level, n in stages:
            levels.append((level, k, n))
            last = level == stages[-1][0]
            for _ in range(n):
                decay = o.lr_final ** (k / total)
                h32 = self.iteration(R, t, images[level], ranges[level], level, decay).numpy()
                h = h32.astype(np.float64)
                loss = float(h[12])
                losses.append(loss)
                if last and loss < best[0]:
                    best = (loss, R, t, h[15:20] if nf == 20 else None, ex32)
                if ex32 is not None:
                    ex32 = h32[nf:nf + 6].copy()  # what the step left: the next iteration's exposure
                R, t = adam.step(h[0:9], h[9:12], decay)
                k += 1
        loss, R, t, gate, ex32 = best
        self._history = (self._history + [(R, t)])[-2:]
        res = TrackResult(rot=R, tran=t, loss=loss, iterations=len(losses), losses=losses)
        if ex32 is not None:
            next(iter(self._exposures.values())).fix()
            self._last_exposure = ex32
            res.exposure = (ex32[0:3].astype(np.float64), ex32[3:6].astype(np.float64))
        if gate is not None:  # (depth pixels, colour pixels, m_d, m_c, n_d) of the returned pose's iteration
            res.inliers = (int(gate[0]), int(gate[4]), int(gate[1]))
            res.medians = (float(gate[2]), float(gate[3]))
        res.levels = levels if self._stages is not None else None
        return res

    # ------------------------------------------------------------------ TrackOptions.device_pose
    MAX_ATTEMPTS = 3

    def _device_buffers(self, rows: int, n_values: int):
        """The device state, ``pose_dev``, the log of ``rows`` rows and ONE pinned host buffer that receives state + log."""
        if self._dp is None or self._dp["rows"] < rows:
            state_bytes = C.sizeof(_lib.GsPoseState)
            state_pad = (state_bytes + 15) // 16 * 16  # (the log behind the state stays 16-byte aligned)
            log_bytes = int(_lib.gs_pose_log_bytes(rows, n_values))
            dev = torch.zeros(state_pad + log_bytes, dtype=torch.uint8, device=self.device)
            self._dp = {"rows": rows, "dev": dev, "state_bytes": state_bytes, "state_pad": state_pad,
                        "pose": torch.zeros(12, dtype=torch.float32, device=self.device),
                        "host": torch.zeros(state_pad + log_bytes, dtype=torch.uint8).pin_memory()}
        return self._dp

    def _stage_list(self, image, range_map):
        """(stages, targets per level, total iterations) of one call -- what ``track`` walks."""
        if self._stages is None:
            stages, images, ranges = ((0, int(self.opt.iterations)),), (image,), (range_map,)
        else:
            stages = self._stages
            images, ranges = self._pyramid.build(image, range_map)
        return stages, images, ranges, sum(n for _, n in stages)

    def _enqueue_device_track(self, R, t, stages, images, ranges, total, dp, n_values):
        """One attempt: reset, then per iteration forward (flagged) / loss / backward_pose / gs_pose_step -- nothing waits."""
        o = self.opt
        base = dp["dev"].data_ptr()
        state_ptr, log_ptr, pose = base, base + dp["state_pad"], dp["pose"]
        rot = (C.c_double * 9)(*np.asarray(R, np.float64).reshape(9))
        tran = (C.c_double * 3)(*np.asarray(t, np.float64).reshape(3))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.call("gs_pose_reset", state_ptr, pose.data_ptr(), log_ptr, total, n_values, rot, tran, stream)
            opts = _lib.GsPoseStepOpts(o.lr_rot, o.lr_tran, 1.0, o.betas[0], o.betas[1], o.eps, 0, n_values)
            k = 0
            for level, n in stages:
                if self._levels is None:
                    r, loss, camera, scale = self.renderer, self.loss, self.camera, 1.0 / (self.H * self.W)
                else:
                    r, loss, camera, scale = self._levels[level]
                opts.track_best = int(level == stages[-1][0])
                for _ in range(n):
                    img, _, depth, alpha = r.forward(*self.params, camera, training=True, aux=True, pose_dev=pose)
                    gi, gd, ga = loss(img, depth, alpha, images[level], ranges[level], scale, values=self._values)
                    r.backward_pose(gi, self._grad_pose, 0, grad_depth=gd, grad_alpha=ga)
                    opts.lr_scale = o.lr_final ** (k / total)
                    _lib.call("gs_pose_step", self._grad_pose[0].data_ptr(), self._grad_pose[1].data_ptr(),
                              self._values.data_ptr(), r.overflow_flag(), C.byref(opts), state_ptr, pose.data_ptr(), log_ptr,
                              total, k, stream)
                    k += 1

    def _read_device_track(self, dp, total, n_values):
        """THE read of a call: state + log into pinned memory, returned as (GsPoseState, log [total, 24 + n_values])."""
        dp["host"].copy_(dp["dev"])  # (device -> pinned host: returns when the bytes have landed)
        raw = dp["host"].numpy()
        state = _lib.GsPoseState.from_buffer_copy(raw[:dp["state_bytes"]].tobytes())
        row_len = _lib.GS_POSE_LOG_HEAD + n_values
        log = raw[dp["state_pad"]:dp["state_pad"] + 4 * row_len * total].view(np.float32).reshape(total, row_len).copy()
        return state, log

    def _track_on_device(self, R, t, image, range_map) -> TrackResult:
        stages, images, ranges, total = self._stage_list(image, range_map)
        n_values = self._values.numel()
        dp = self._device_buffers(total, n_values)
        renderers = [self.renderer] if self._levels is None else [lv[0] for lv in self._levels.values()]
        for attempt in range(1, self.MAX_ATTEMPTS + 1):
            self._enqueue_device_track(R, t, stages, images, ranges, total, dp, n_values)
            state, log = self._read_device_track(dp, total, n_values)
            if state.skipped == 0:
                break
            # a frame overflowed its workspace (rendered empty, its step skipped on the device): grow by the renderer's own
            # rule -- its counters are those of its LAST frame, which is enough to know a larger capacity -- and start over
            if attempt == self.MAX_ATTEMPTS:
                raise RuntimeError(f"Tracker.track(device_pose): frames still overflow their workspace after {attempt} attempts "
                                   f"(max_pairs {[r.max_pairs for r in renderers]})")
            k = 0
            for level, n in stages:
                if np.isnan(log[k:k + n, _lib.GS_POSE_LOG_HEAD]).any():  # (a skipped row's loss is NaN)
                    r = self.renderer if self._levels is None else self._levels[level][0]
                    st = r.stats()  # (its last frame's counters: the pairs that frame needed, if it overflowed too)
                    r.max_pairs = max(int(st.overflow * r.headroom) + 1024, 2 * r.max_pairs)
                k += n
        # (an iteration whose loss or gradient was not finite took no step and competes for nothing: its row shows it)
        levels, k = [], 0
        for level, n in stages:
            levels.append((level, k, n))
            k += n
        Rb = np.array(state.best_R, np.float64).reshape(3, 3)
        tb = np.array(state.best_t, np.float64)
        losses = [float(x) for x in log[:, _lib.GS_POSE_LOG_HEAD]]
        self._history = (self._history + [(Rb, tb)])[-2:]
        res = TrackResult(rot=Rb, tran=tb, loss=float(state.best_loss), iterations=total, losses=losses)
        res.attempts = attempt
        if n_values == 8 and state.best_row >= 0:  # (depth pixels, colour pixels, m_d, m_c, n_d) of the best row
            gate = log[state.best_row, _lib.GS_POSE_LOG_HEAD + 3:_lib.GS_POSE_LOG_HEAD + 8]
            res.inliers = (int(gate[0]), int(gate[4]), int(gate[1]))
            res.medians = (float(gate[2]), float(gate[3]))
        res.levels = levels if self._stages is not None else None
        res.log = log  # [iterations, 24 + n_values]: per row the pose rendered, dL/drot, dL/dtran and the loss's values
        return res
