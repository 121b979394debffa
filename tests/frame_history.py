"""The catalogue behind tests/test_frame_history_host.py and tests/test_gpu_frame_history.py: scenes, cameras, modes and the
HISTORIES -- lists of (scene, camera, mode) that ONE FrameRenderer renders in that order.  GPU-free: everything here is NumPy
and the oracle, so that the host tier can prove on the CPU that every frame is a valid input and that the histories contain
every transition they are meant to contain (``transitions``), and the GPU tier only asserts kernels and caches.

The property the GPU tier pins: frame k of any history equals, bit for bit, frame k rendered alone by a renderer that has
seen nothing else.

All scenes are make_scene(..., 128, 96, ...): the focal length of every camera is 0.75 W, so each of them sees the same
frustum filled.  Scenes are handed out as NumPy arrays and turned into tensors once per history (``history_tensors``): tensor
identity is part of a history (A2000 is a view of A's tensors: the same address, another N)."""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

from gs_scene import Camera, Scene, make_camera, make_scene

W0, H0 = 128, 96
MAX_PAIRS = 1 << 18
SMALL_PAIRS = 4096  # the capacity histories start here: TINY fits, A does not

# ---------------------------------------------------------------------------------------------------------------- scenes
PILE_COUNT, PILE_OPA, PILE_DEPTH, PILE_PX_SIGMA = 2_100, 6.0, 9.0, 100.0
SCENES = ("A", "A2000", "B", "SH2", "SH3", "TINY", "PILE", "BIG")


def _rows(sc: Scene, n: int) -> Scene:
    return Scene(sc.pos[:n], sc.quat[:n], sc.scale[:n], sc.opa[:n], sc.rgb[:n])


def _more_opaque(sc: Scene, shift: float) -> Scene:
    sc.opa = (sc.opa + np.float32(shift)).astype(np.float32)
    return sc


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    """The scene ``name``, computed once and shared: read only."""
    if name == "A":
        # (opacity logits + 1: every tile of C1 saturates and an occlusion-culled frame emits under half of the pairs -- well
        # inside what the renderer's policy keeps the cull for, CULL_MIN_GAIN = 0.65; the host tier restates the estimate)
        return _more_opaque(make_scene(6_000, W0, H0, seed=7), 1.0)
    if name == "A2000":
        return _rows(scene("A"), 2_000)
    if name == "B":
        return make_scene(6_000, W0, H0, seed=8)
    if name == "SH2":
        return make_scene(3_000, W0, H0, seed=9, use_sh=True, sh_degree=2)
    if name == "SH3":
        return make_scene(3_000, W0, H0, seed=10, use_sh=True, sh_degree=3)
    if name == "TINY":
        return make_scene(37, W0, H0, seed=11)
    if name == "BIG":
        # (opacity logits + 2: the longest list is beyond 2,048, the longest WALK well below: no segmented compositing)
        return _more_opaque(make_scene(140_000, W0, H0, seed=12, max_px_sigma=2.0), 2.0)
    if name == "PILE":
        # A2000 plus PILE_COUNT opaque Gaussians stacked on the central pixel, behind most of the scene.  Their footprint
        # (PILE_PX_SIGMA pixels) covers the whole frame with a weight above 0.7, so every tile lists all of them -- lists beyond
        # the per-tile sort's window -- and every pixel saturates within a few of them: the WALK stays short.
        base = scene("A2000")
        rng = np.random.default_rng(13)
        k = PILE_COUNT
        pos = np.zeros((k, 3), np.float32)
        pos[:, 2] = PILE_DEPTH + np.sort(rng.uniform(0.0, 0.5, k)).astype(np.float32)
        sigma = np.float32(PILE_PX_SIGMA * PILE_DEPTH / (0.75 * W0))
        scale = np.full((k, 3), sigma, np.float32)
        quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (k, 1))
        opa = np.full(k, PILE_OPA, np.float32)
        rgb = rng.normal(0.0, 1.0, (k, 3)).astype(np.float32)
        cat = lambda a, b: np.ascontiguousarray(np.concatenate([a, b], 0), np.float32)  # noqa: E731
        return Scene(cat(base.pos, pos), cat(base.quat, quat), cat(base.scale, scale), cat(base.opa, opa), cat(base.rgb, rgb))
    raise KeyError(name)


def history_tensors(history, device):
    """{scene name: [pos, quat, scale, opa, rgb] on ``device``} for the scenes ``history`` uses, made once: the tensors'
    identity is part of the history.  A2000's tensors are the first 2,000 rows of A's, as views."""
    from gs_testutil import to_torch

    names = {s.scene for s in history.steps}
    out = {}
    if names & {"A", "A2000"}:
        out["A"] = to_torch(scene("A"), device)
        out["A2000"] = [t[:2_000] for t in out["A"]]
        assert all(v.data_ptr() == t.data_ptr() and v.is_contiguous() for v, t in zip(out["A2000"], out["A"]))
    for name in sorted(names - {"A", "A2000"}):
        out[name] = to_torch(scene(name), device)
    return {k: v for k, v in out.items() if k in names}


# --------------------------------------------------------------------------------------------------------------- cameras
CAMERAS = ("C1", "C1near", "C1mid", "C1far", "C2", "C3", "C4", "C5", "C6")
YAW = {"C1": 0.0, "C1near": 0.2, "C1mid": 3.0, "C1far": 10.0}
SIZE = {"C2": (64, 48), "C3": (50, 37), "C4": (40, 200)}
MUTABLE = "CM@"  # "CM@C1mid": the history's ONE mutable Camera object, its rot / tran overwritten in place with C1mid's


def camera(name: str) -> Camera:
    """A fresh Camera object for ``name`` (``CM@X``: X's)."""
    from gs_testutil import general_camera
    from pp_testutil import OFFSETS, offset_camera

    name = pose_name(name)
    if name in YAW:
        return make_camera(W0, H0, yaw_deg=YAW[name])
    if name in SIZE:
        return make_camera(*SIZE[name])
    if name == "C5":
        return general_camera(W0, H0)
    if name == "C6":
        return offset_camera(make_camera(W0, H0), OFFSETS[0])
    raise KeyError(name)


def pose_name(name: str) -> str:
    return name[len(MUTABLE):] if name.startswith(MUTABLE) else name


class HistoryCameras:
    """The Camera objects of one history: one object per name, handed out again whenever the name comes back (a trainer's
    fixed camera set), and one mutable object behind every ``CM@X`` step, overwritten in place (a viewer's)."""

    def __init__(self):
        self._cams = {}
        self._mutable = None

    def get(self, name: str) -> Camera:
        if name.startswith(MUTABLE):
            src = camera(name)
            if self._mutable is None:
                self._mutable = src
            else:
                self._mutable.rot[...] = src.rot
                self._mutable.tran[...] = src.tran
            return self._mutable
        if name not in self._cams:
            self._cams[name] = camera(name)
        return self._cams[name]


def camera_shift_px(prev: Camera, cur: Camera) -> float:
    """FrameRenderer._camera_shift_px restated: rotation angle x focal length + focal length x centre displacement at unit
    depth; infinite between cameras of another size, focal length or principal point."""
    same = (prev.width, prev.height, prev.focal_x, prev.focal_y, prev.cx, prev.cy) == \
        (cur.width, cur.height, cur.focal_x, cur.focal_y, cur.cx, cur.cy)
    if not same:
        return float("inf")
    r0, t0 = np.asarray(prev.rot, np.float32).astype(np.float64), np.asarray(prev.tran, np.float32).astype(np.float64)
    r1, t1 = np.asarray(cur.rot, np.float32).astype(np.float64), np.asarray(cur.tran, np.float32).astype(np.float64)
    ang = float(np.linalg.norm(r1 - r0) / np.sqrt(2.0))
    dc = float(np.linalg.norm(r1.T @ t1 - r0.T @ t0))
    return max(float(cur.focal_x), float(cur.focal_y)) * (ang + dc)


# ----------------------------------------------------------------------------------------------------------------- modes
# I: inference; Ia: inference with aux; T: training forward, backward never called; Tb: training forward + backward;
# Tab: aux training + backward with grad_depth and grad_alpha; Tp: training + backward with grad_pose (rgb only)
MODES = ("I", "Ia", "T", "Tb", "Tab", "Tp")
TRAINING = {"T", "Tb", "Tab", "Tp"}
AUX = {"Ia", "Tab"}


@dataclass(frozen=True)
class Step:
    scene: str
    camera: str
    mode: str

    def colour_dim(self) -> int:
        return int(scene(self.scene).rgb.shape[1])

    def shape(self):
        c = camera(self.camera)
        return (scene(self.scene).n, c.width, c.height, self.colour_dim())


@dataclass
class History:
    name: str
    steps: list
    max_pairs: int = MAX_PAIRS
    auto_grow: tuple = (True, "async", False)  # the settings the history allows
    overflow: tuple = ()   # indices of the steps that need more than the capacity they meet
    grows: bool = False    # ... and the renderer grows there (auto_grow True / "async" on a checked frame)
    about: frozenset = field(default_factory=frozenset)  # the regimes the GPU tier asserts it crossed

    def has_backward(self) -> bool:
        return any(s.mode in ("Tb", "Tab", "Tp") for s in self.steps)


def _steps(text: str) -> list:
    """"A C1 I, A C2 I" -> [Step, Step]"""
    return [Step(*part.split()) for part in text.split(",") if part.strip()]


def _size_walk(mode):
    cams = ["C1", "C2", "C1", "C2", "C3", "C2", "C1", "C4", "C1", "C5", "C6", "C1"]
    return [Step("A", c, mode) for c in cams]


def _count_walk(mode):
    return [Step(s, "C1", mode) for s in ["A", "A2000", "A", "B", "A", "TINY", "A"]]


def _shuffled(seed: int, n: int) -> list:
    """A seeded walk over the small scenes, all cameras and all modes (Tp on rgb scenes only)."""
    rng = np.random.default_rng(seed)
    scenes, cams = ["A", "A2000", "B", "SH2", "SH3", "TINY"], ["C1", "C2", "C3", "C4", "C5", "C6"]
    out = []
    for _ in range(n):
        s = scenes[int(rng.integers(len(scenes)))]
        c = cams[int(rng.integers(len(cams)))]
        modes = [m for m in MODES if not (m == "Tp" and s in ("SH2", "SH3"))]
        out.append(Step(s, c, modes[int(rng.integers(len(modes)))]))
    return out


_REST = "A C1 I, A C1 I, A C1 I, A C1near I, A C1mid I, A C1far I, A C1 I"
_REST_BROKEN = "A C1 I, A C1 I, A C2 I, A C1 I, A C1near I, A C1mid I, A C1far I, A C1 I"

HISTORIES = {h.name: h for h in (
    History("size_I", _size_walk("I")),
    History("size_Tb", _size_walk("Tb")),
    History("count_I", _count_walk("I")),
    History("count_Tb", _count_walk("Tb")),
    History("big", _steps("A C1 I, BIG C1 I, A C1 I, BIG C1 Tb, A C1 Tb"), max_pairs=1 << 20, about=frozenset({"big"})),
    History("colour", _steps("A C1 I, SH2 C1 I, SH3 C1 I, A C1 I, SH3 C1 I, A C1 I, "
                             "A C1 Tb, SH2 C1 Tb, SH3 C1 Tb, A C1 Tb, SH3 C1 Tb, A C1 Tb")),
    # an Euler tour of the twelve ordered pairs of (I, Ia, T, Tab), then Tb / Tab / Tp right behind a T of another shape
    History("modes", _steps("A C1 I, A C1 Ia, A C1 T, A C1 Tab, A C1 I, A C1 T, A C1 I, A C1 Tab, A C1 T, A C1 Ia, A C1 Tab, "
                            "A C1 Ia, A C1 I, A C2 T, A C1 Tb, SH2 C1 T, A C1 Tab, A C4 T, A C1 Tp")),
    History("rest", _steps(_REST), about=frozenset({"cull", "far"})),
    History("rest_broken", _steps(_REST_BROKEN), about=frozenset({"cull", "far", "reshape"})),
    History("rest_long", _steps(", ".join(["A C1 I"] * 7)), about=frozenset({"repeat"})),
    History("viewer", _steps("A CM@C1 I, A CM@C1 I, A CM@C1near I, A CM@C1mid I, A CM@C1 I, A CM@C1far I, SH2 CM@C1far I, "
                             "SH2 CM@C1 I"), about=frozenset({"viewer"})),
    History("pile", _steps("PILE C1 I, A C1 I, SH2 C1 I, A C2 I, PILE C1 Tb, A C1 Tb"), about=frozenset({"pile"})),
    History("grow", _steps("TINY C1 I, A C1 I, TINY C1 I, TINY C2 Tb"), max_pairs=SMALL_PAIRS, auto_grow=(True, "async"),
            overflow=(1,), grows=True, about=frozenset({"grow"})),
    History("overflow", _steps("TINY C1 T, A C1 T, TINY C1 I, TINY C1 Tb"), max_pairs=SMALL_PAIRS, auto_grow=(False, "async"),
            overflow=(1,), about=frozenset({"overflow"})),
    History("shuffle_1", _shuffled(101, 16)),
    History("shuffle_2", _shuffled(202, 16)),
)}


# ------------------------------------------------------------------------------------------------------------ transitions
def _find(names, pattern):
    """Does the list ``names`` contain ``pattern`` as a run of consecutive items?"""
    return any(names[k:k + len(pattern)] == pattern for k in range(len(names) - len(pattern) + 1))


def transitions(history: History) -> set:
    """The transitions of the catalogue's list that ``history`` contains, as tuples -- computed from its steps alone."""
    out = set()
    st = history.steps
    for a, b in zip(st, st[1:]):
        ca, cb = pose_name(a.camera), pose_name(b.camera)
        (na, wa, ha, da), (nb, wb, hb, db) = a.shape(), b.shape()
        same_scene, same_cam = a.scene == b.scene, ca == cb
        if same_scene and (wa, ha) != (wb, hb) and a.mode == b.mode and a.mode in ("I", "Tb"):
            out.add(("size", ca, cb, a.mode))
        if same_cam and not same_scene and da == db:
            out.add(("count", a.scene, b.scene))
        if same_cam and da != db:
            out.add(("colour", a.scene, b.scene))
        if same_scene and same_cam and a.mode != b.mode and {a.mode, b.mode} <= {"I", "Ia", "T", "Tab"}:
            out.add(("mode", a.mode, b.mode))
        if a.mode == "T" and b.mode in ("Tb", "Tab", "Tp") and a.shape() != b.shape():
            out.add(("behind_an_open_T", b.mode))
        if a.camera.startswith(MUTABLE) and b.camera.startswith(MUTABLE) and ca != cb:
            out.add(("camera_in_place",))
    plain = [f"{s.scene} {pose_name(s.camera)} {s.mode}" for s in st if not s.camera.startswith(MUTABLE)]
    if _find(plain, [p.strip() for p in _REST.split(",")]):
        out.add(("rest_near_mid_far_back",))
    rb = [p.strip() for p in _REST_BROKEN.split(",")]
    if _find(plain, rb) and camera(rb[2].split()[1]).width != W0:
        out.add(("rest_interrupted_near_mid_far_back",))
    if True in history.auto_grow:
        names = [(s.scene, pose_name(s.camera)) for s in st]
        if ("PILE", "C1") in names:
            behind = names[names.index(("PILE", "C1")) + 1:]
            out |= {("behind_pile", "A")} if ("A", "C1") in behind else set()
            out |= {("behind_pile", "SH2")} if ("SH2", "C1") in behind else set()
            out |= {("behind_pile", "C2")} if any(c == "C2" for _, c in behind) else set()
    for k in history.overflow:
        if k + 1 < len(st) and scene(st[k + 1].scene).n < scene(st[k].scene).n:
            out.add(("grown_then_small",) if history.grows else ("overflowed_then_clean",))
    return out


# ----------------------------------------------------------------------------------------------------------- oracle side
@functools.lru_cache(maxsize=None)
def oracle_frame(scene_name: str, camera_name: str):
    """The oracle's frame of (scene, camera), computed once per process and shared: read only."""
    from gs_testutil import OracleFrame
    from pp_testutil import PPOracleFrame

    cam = camera(camera_name)
    cls = PPOracleFrame if cam.cx is not None else OracleFrame
    return cls(copy.copy(scene(scene_name)), cam)


def distinct_frames(histories=None) -> list:
    """Every distinct (scene, camera) the histories use, sorted."""
    hs = HISTORIES.values() if histories is None else histories
    return sorted({(s.scene, pose_name(s.camera)) for h in hs for s in h.steps})


def walk_lengths_f64(of) -> np.ndarray:
    """[tiles] the longest walk of each tile of the oracle frame ``of``, restated in float64: a pixel takes a step for every
    entry of its tile's list that finds its transmittance at 1e-4 or above (alpha = opacity x exp(q), T *= 1 - alpha); a
    tile's walk is that of its slowest pixel."""
    g = of.grid
    ntx = g.padded_width // 16
    n_tiles = len(of.accum) - 1
    out = np.zeros(n_tiles, np.int64)
    fx, fy = float(g.focal_x), float(g.focal_y)
    for t in range(n_tiles):
        lo, hi = int(of.accum[t]), int(of.accum[t + 1])
        if hi == lo:
            continue
        ty, tx = divmod(t, ntx)
        xs = (np.arange(16) + 16 * tx + 0.5 - g.padded_width // 2) / fx
        ys = (np.arange(16) + 16 * ty + 0.5 - g.padded_height // 2) / fy
        px, py = (a.reshape(-1, 1) for a in np.meshgrid(xs, ys))
        pos, cov, opa = (np.asarray(a[lo:hi], np.float64) for a in (of.s_pos, of.s_cov, of.s_opa))
        a, b, c, d = cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 3]
        x, y = px - pos[:, 0], py - pos[:, 1]
        q = -(d * x * x - (b + c) * x * y + a * y * y) / (2.0 * (a * d - b * c) + 1e-14)
        alpha = opa * np.exp(q)
        before = np.concatenate([np.ones((256, 1)), np.cumprod(1.0 - alpha, axis=1)[:, :-1]], axis=1)
        out[t] = int((before >= 1e-4).sum(axis=1).max())
    return out


def cull_emitted_share_f64(of) -> float:
    """An estimate of the share of ``of``'s pairs that an occlusion-culled repeat of the frame still emits: a tile whose
    every pixel stops inside its list keeps the entries up to 1.0625 x the depth of the entry its slowest pixel stopped at
    (the cut the compositing launch leaves behind), any other tile keeps its whole list."""
    walk, lens = walk_lengths_f64(of), np.diff(of.accum)
    kept = 0
    for t in range(len(lens)):
        lo, hi = int(of.accum[t]), int(of.accum[t + 1])
        if lens[t] == 0 or walk[t] >= lens[t]:
            kept += int(lens[t])
            continue
        d = of.s_pos[lo:hi, 2].astype(np.float64)
        kept += int((d <= 1.0625 * d[walk[t] - 1]).sum())
    return kept / max(len(of.ids), 1)
