"""Frame-to-model point-to-plane ICP: the pose of an incoming depth frame against the map's own depth, solved on the device.

The second, classical answer of an RGB-D pipeline to "where is the camera", beside the photometric descent of
``gs_track.Tracker``.  The map is rendered ONCE, at the predicted pose (``FrameRenderer.forward(..., aux=True)``: depth and
alpha); ``IcpAligner.set_model`` turns those maps into a vertex map and a normal map (gs_icp_model_maps, csrc/icp.hip).  After
that an iteration is one pass over the incoming range map and a 6 x 6 solve (gs_icp_step: two launches, no atomics): no
rendering, no backward, and -- because the solve and the pose update run on the device -- no host read.  ``align`` enqueues
the whole coarse-to-fine schedule and reads the state and the log back once.

The per-pixel rule is stated in include/gs_abi.h and csrc/icp_point.h: nearest-pixel projective association, central-difference
normals that stop at depth edges, a distance gate and a grazing-angle gate.  There is no colour term and no test on the
incoming frame's own normals.

What ICP cannot see: a scene that does not constrain all six degrees of freedom.  A corner whose third plane has left the view
lets the camera slide along the remaining edge with a residual as small as a converged one (tests/test_icp_host.py asserts
this).  ``IcpResult`` therefore carries the counts and the whole log, and ``accepted`` is a necessary test, not a sufficient
one.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

import gs_seed
from gaussian import _lib
from gs_call import check_tensor, require_hip, stream, workspace
from gs_geometry import pose64
from gs_track import so3_exp

LOG_DOUBLES = _lib.GS_ICP_LOG_DOUBLES
_STATE_DOUBLES = 16  # struct gs_icp_state (104 bytes) in front of the log, padded to 128


@dataclass
class IcpOptions:
    """Which defaults have evidence: ``stages`` -- (stride, iterations), coarse first, KinectFusion's 4 / 5 / 10 -- and
    ``dist_max`` = 0.2 bring the analytic room corner of tests/icp_ref.py from 0.5 to 8 degrees off to below a tenth of the
    start error, in a float64 restatement and on the device, and that is all the evidence there is: one synthetic scene, exact
    ranges.  ``cos_min`` = 0 (no grazing test beyond the normal facing the camera), ``damping`` = 1e-6, ``alpha_min`` = 0.5
    (the Tracker's silhouette), ``edge_rel`` = 0.1 (the pyramid's arbitrary value), ``normal_step`` = 1,
    ``min_inlier_share`` = 0.25 and ``min_count`` = 6 (the number of unknowns) have none."""
    stages: Tuple[Tuple[int, int], ...] = ((4, 4), (2, 5), (1, 10))
    dist_max: float = 0.2
    cos_min: float = 0.0
    damping: float = 1e-6
    alpha_min: float = 0.5
    edge_rel: float = 0.1
    normal_step: int = 1
    min_inlier_share: float = 0.25
    min_count: int = 6

    def validated(self) -> Tuple[Tuple[int, int], ...]:
        """``stages`` as a tuple of (stride, iterations) ints; raises ValueError for what the library would refuse and for an
        empty or malformed schedule."""
        out = []
        for stage in self.stages:
            if len(stage) != 2 or any(int(x) != x for x in stage):
                raise ValueError(f"stages holds pairs (stride, iterations) of integers, got {stage!r}")
            stride, n = int(stage[0]), int(stage[1])
            if stride < 1 or n < 1:
                raise ValueError(f"a stage needs stride >= 1 and iterations >= 1, got {stage!r}")
            out.append((stride, n))
        if not out:
            raise ValueError("stages is empty: at least one (stride, iterations)")
        if not self.dist_max > 0.0:
            raise ValueError(f"dist_max must be positive, got {self.dist_max}")
        if self.cos_min != self.cos_min or self.alpha_min != self.alpha_min or self.edge_rel != self.edge_rel:
            raise ValueError("cos_min, alpha_min and edge_rel must not be NaN")
        if not (self.damping >= 0.0 and math.isfinite(self.damping)):
            raise ValueError(f"damping must be finite and not negative, got {self.damping}")
        if int(self.normal_step) < 1:
            raise ValueError(f"normal_step must be >= 1, got {self.normal_step}")
        if not 0.0 <= self.min_inlier_share <= 1.0:
            raise ValueError(f"min_inlier_share must lie in [0, 1], got {self.min_inlier_share}")
        if int(self.min_count) < 0:
            raise ValueError(f"min_count must not be negative, got {self.min_count}")
        return tuple(out)


@dataclass
class IcpResult:
    rot: np.ndarray        # [3,3] float64, the frame's world -> camera pose (the ``init`` pose when not accepted)
    tran: np.ndarray       # [3] float64
    iterations: int
    rmse: float            # sqrt(sum e e / kept) of the last iteration, taken before its own step
    inliers: int           # kept pixels of the last iteration
    measured: int          # measured lattice pixels of the last iteration
    accepted: bool
    log: np.ndarray = field(default_factory=lambda: np.zeros((0, LOG_DOUBLES)))  # [iterations, GS_ICP_LOG_DOUBLES]
    relative: Optional[Tuple[np.ndarray, np.ndarray]] = None  # (R, t) the device ended with: p_model = R p_frame + t


def so3_log(R) -> np.ndarray:
    """w with exp([w]x) = R, in float64 (angles below pi)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    s = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5  # sin(th) axis
    n = float(np.linalg.norm(s))
    th = math.atan2(n, (float(np.trace(R)) - 1.0) * 0.5)
    if n < 1e-12:
        return s
    return s * (th / n)


def _on_so3(R) -> np.ndarray:
    """R back onto SO(3) through so3_exp; beyond 3 rad, where the logarithm loses its axis, through the polar factor."""
    w = so3_log(R)
    if float(np.linalg.norm(w)) > 3.0:
        U, _, Vt = np.linalg.svd(np.asarray(R, np.float64).reshape(3, 3))
        return U @ Vt
    return so3_exp(w)


def relative_pose(rot_m, tran_m, rot_f, tran_f):
    """(R, t) with p_model = R p_frame + t for the world -> camera poses of the model view and of the frame, in float64."""
    (rot_m, tran_m), (rot_f, tran_f) = pose64(rot_m, tran_m), pose64(rot_f, tran_f)
    R = _on_so3(rot_m @ rot_f.T)
    return R, tran_m - R @ tran_f


def compose(rot_m, tran_m, R, t):
    """The frame's world -> camera pose from the model view's pose and (R, t): rot = R^T rot_m, tran = R^T (tran_m - t), in
    float64, rot re-orthonormalised through so3_exp."""
    (rot_m, tran_m), (R, t) = pose64(rot_m, tran_m), pose64(R, t)
    return _on_so3(R.T @ rot_m), R.T @ (tran_m - t)


def decide(log: np.ndarray, min_inlier_share: float) -> bool:
    """``IcpResult.accepted`` from the log alone (host only): false when an iteration reported a failed solve, when the
    last iteration's inlier share is below ``min_inlier_share``, or when the last rmse exceeds the first iteration's."""
    log = np.asarray(log, np.float64).reshape(-1, LOG_DOUBLES)
    if len(log) == 0 or np.any(log[:, 36] != _lib.GS_ICP_OK):
        return False
    kept, measured = log[:, 0], log[:, 1]
    if measured[-1] <= 0 or kept[-1] < float(min_inlier_share) * measured[-1]:
        return False
    rmse = np.sqrt(log[:, 2] / np.maximum(kept, 1.0))
    return bool(rmse[-1] <= rmse[0])


def _read(host: torch.Tensor, dev: torch.Tensor):
    """The one synchronising copy of ``align`` (device -> pinned host); the tests count its calls."""
    host.copy_(dev)


class IcpAligner:
    """``IcpAligner(camera, options, device)``: ``camera`` gives the size, the focal lengths and the principal point of the
    incoming frames.  ``set_model(depth, alpha, rot, tran)`` builds the vertex and normal maps of the map as rendered from the
    world -> camera pose (rot, tran) -- ``alpha`` None: ``depth`` is a plain range map --, one launch into buffers allocated
    once per model size.  ``align(range_map, init)`` estimates the frame's pose: reset + two launches per iteration on the
    current stream, then ONE read of the state and the log."""

    def __init__(self, camera, options: Optional[IcpOptions] = None, device="cuda"):
        self.opt = options if options is not None else IcpOptions()
        self._stages = self.opt.validated()
        self.device = require_hip(device, "IcpAligner")
        self.camera = camera
        self._cam = gs_seed.seed_camera_pp(camera)
        self._rows = sum(n for _, n in self._stages)
        o = self.opt
        self._mopts = _lib.GsIcpModelOpts(float(o.alpha_min), float(o.edge_rel), int(o.normal_step))
        # the state (padded to 128 bytes) and the log in ONE buffer, so that one copy brings both
        n = _STATE_DOUBLES + self._rows * LOG_DOUBLES
        self._dev = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._host = torch.zeros(n, dtype=torch.float64).pin_memory()
        self._ws = {}        # stride -> workspace of gs_icp_step for the frame's size
        self._model = None   # (vertex, normal, GsSeedCameraPP, rot, tran)
        self._maps = {}      # (H, W) -> (vertex, normal)

    def _workspace(self, cam, stride: int) -> torch.Tensor:
        key = (cam.cam.height, cam.cam.width, stride)
        if key not in self._ws:
            self._ws[key] = workspace(_lib.gs_icp_workspace_bytes(*key), self.device, floor=256)
        return self._ws[key]

    def set_model(self, depth: torch.Tensor, alpha: Optional[torch.Tensor], rot, tran, camera=None):
        """``depth`` / ``alpha`` [H,W]: the map's depth and alpha maps as ``render_aux`` returns them, from the world -> camera
        pose (rot, tran) through ``camera`` (default: the aligner's); ``alpha`` None: ``depth`` is a range map.  Returns
        (vertex, normal) [H,W,4] -- overwritten by the next call of the same size."""
        cam = gs_seed.seed_camera_pp(camera if camera is not None else self.camera)
        H, W = cam.cam.height, cam.cam.width
        check_tensor("depth", depth, (H, W))
        if alpha is not None:
            check_tensor("alpha", alpha, (H, W))
        if (H, W) not in self._maps:
            self._maps[(H, W)] = tuple(torch.empty((H, W, 4), dtype=torch.float32, device=self.device) for _ in range(2))
        vertex, normal = self._maps[(H, W)]
        with torch.cuda.device(self.device):
            _lib.call("gs_icp_model_maps", depth.data_ptr(), alpha.data_ptr() if alpha is not None else None, C.byref(cam),
                      C.byref(self._mopts), vertex.data_ptr(), normal.data_ptr(), stream())
        self._model = (vertex, normal, cam, *pose64(rot, tran))
        return vertex, normal

    def align(self, range_map: torch.Tensor, init=None, camera=None) -> IcpResult:
        """``range_map`` [H,W]: the incoming frame's range (<= 0, inf, NaN: no measurement).  ``init`` = (rot, tran): where the
        frame is believed to be (world -> camera); default: the model view's pose, so the relative motion starts at the
        identity.  ``camera``: the frame's camera where it differs from the aligner's."""
        if self._model is None:
            raise RuntimeError("align() needs a model: call set_model() first")
        vertex, normal, mcam, rot_m, tran_m = self._model
        cam = gs_seed.seed_camera_pp(camera) if camera is not None else self._cam
        check_tensor("range_map", range_map, (cam.cam.height, cam.cam.width))
        if init is None:
            rot0, tran0 = rot_m, tran_m
            R0, t0 = np.eye(3), np.zeros(3)
        else:
            rot0, tran0 = pose64(*init)
            R0, t0 = relative_pose(rot_m, tran_m, rot0, tran0)
        o = self.opt
        state, log = self._dev[:_STATE_DOUBLES], self._dev[_STATE_DOUBLES:]
        R9, t3 = (C.c_double * 9)(*R0.reshape(9)), (C.c_double * 3)(*t0)
        with torch.cuda.device(self.device):
            s = stream()
            _lib.call("gs_icp_reset", state.data_ptr(), log.data_ptr(), self._rows, R9, t3, s)
            row = 0
            for stride, n in self._stages:
                ws = self._workspace(cam, stride)
                opts = _lib.GsIcpOpts(stride, float(o.dist_max), float(o.cos_min), int(o.min_count), float(o.damping))
                for _ in range(n):
                    _lib.call("gs_icp_step", range_map.data_ptr(), C.byref(cam), vertex.data_ptr(), normal.data_ptr(),
                              C.byref(mcam), C.byref(opts), state.data_ptr(), log.data_ptr(), self._rows, row, ws.data_ptr(),
                              ws.numel(), s)
                    row += 1
            _read(self._host, self._dev)
        h = self._host.numpy()
        R, t = h[0:9].reshape(3, 3).copy(), h[9:12].copy()
        rows = h[_STATE_DOUBLES:].reshape(self._rows, LOG_DOUBLES).copy()
        accepted = decide(rows, o.min_inlier_share)
        last = rows[-1]
        rot, tran = compose(rot_m, tran_m, R, t) if accepted else (rot0.copy(), tran0.copy())
        return IcpResult(rot=rot, tran=tran, iterations=self._rows,
                         rmse=math.sqrt(last[2] / last[0]) if last[0] > 0 else math.inf, inliers=int(last[0]),
                         measured=int(last[1]), accepted=accepted, log=rows, relative=(R, t))
