"""The delayed-producer harness and the catalogue of stream-order cases (no tests in here; nothing touches the GPU at import).

Every entry point of include/gs_abi.h that enqueues work takes a ``gs_stream_t`` and promises to launch everything on it.  On
the default stream a launch that went to the wrong stream still lands in its producer's queue and returns the right bits, so
the suite's default-stream tests cannot see it.  ``run_case`` runs a *case* twice:

  baseline   default stream, no delay: a warm-up call on DECOY inputs (workspaces, per-object state), the TRUE inputs copied
             in, the call, the outputs read back as bytes;
  delayed    everything on one ``torch.cuda.Stream()`` S (chosen once per session, ``choose_streams``: one this runtime does not
             serialise behind the default stream): a fresh object, the same warm-up, then -- in order on S -- a delay
             kernel, ``input.copy_(true)`` for every input, the call, ``output.clone()`` for every output, and
             ``input.copy_(decoy)`` again.  The snapshot must equal the baseline's bytes, carried state included.

A kernel, memset or copy that ignored S runs while the delay still holds the true inputs back: it reads the decoy and the
snapshot differs.  The trailing decoy copy catches work still reading on a stream that was never joined back; a correct
library cannot fail on it.  Decoys are valid inputs -- another scene of the same shapes, other images, zero counts --, so a
misrouted kernel computes a wrong answer inside its bounds.

Two assertions keep the harness from hiding a failure: the delay held (``S.query()`` is False right after the call returned,
except for the cases listed as synchronising, with the sentence that says so), and the harness can see (``positive_control``).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_abi.h")

DELAY_MS_MIN = 40.0   # the delay of a case whose Python call takes up to 2 ms of host time
DELAY_MS_MAX = 200.0  # ... and the most a case may wait
DELAY_FACTOR = 20.0   # delay >= this x the host time of the case's own call, measured in its baseline run


def stream_entry_points(path: str = HEADER) -> List[str]:
    """Every prototype of the header whose parameter list ends in ``gs_stream_t stream)``, in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(gs_\w+)\s*\(([^;{}()]*?)gs_stream_t\s+stream\s*\)\s*;", text)]


# ---------------------------------------------------------------------------------------------------- a case and its run
class Run:
    """One object under test with its device inputs.  ``input`` registers a tensor that the harness fills with the decoy, then
    (late) with the true values; ``call`` issues the library calls on the CURRENT stream and returns {name: output tensor}.
    Names that start with ``state:`` are carried state (read and written): they are compared but not filled with the sentinel.
    ``check`` (optional) runs after the baseline's synchronisation: what the case needs to be true to mean anything."""

    def __init__(self, device):
        self.device = device
        self.inputs: Dict[str, tuple] = {}
        self.call: Callable[[], dict] = None
        self.extra_streams: list = []   # further streams the case itself issues on (joined back into S inside ``call``)
        self.check: Optional[Callable[[], None]] = None
        self.canon: Dict[str, Callable[[np.ndarray], np.ndarray]] = {}  # output name -> canonical form (atomic order)

    def input(self, name, true, decoy, into=None):
        import torch

        true, decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert true.shape == decoy.shape and true.dtype == decoy.dtype, name
        assert true.size == 0 or true.tobytes() != decoy.tobytes(), f"{name}: the decoy equals the true input"
        staged = [torch.from_numpy(a.copy()).to(self.device) for a in (true, decoy)]
        cur = staged[1].clone() if into is None else into
        assert tuple(cur.shape) == true.shape and cur.is_contiguous(), name
        cur.copy_(staged[1])
        self.inputs[name] = (cur, staged[0], staged[1])
        return cur


@dataclass
class Case:
    name: str
    build: Callable[[object], Run]
    covers: Tuple[str, ...]
    synchronising: Optional[str] = None  # the sentence of gs_abi.h or of the class's docstring that says the call waits


@dataclass
class Session:
    """What is calibrated once per session, and what the cases report (profiles/stream_order.txt is written from it)."""
    delay: Callable[[float], None] = None
    S: object = None    # the stream of every delayed run, and a second one (choose_streams)
    S2: object = None
    kind: str = ""
    unit_per_ms: float = 0.0
    notes: List[str] = field(default_factory=list)
    host_ms: Dict[str, float] = field(default_factory=dict)
    delay_ms: Dict[str, float] = field(default_factory=dict)
    wall_s: Dict[str, float] = field(default_factory=dict)


def _elapsed(fn) -> float:
    import torch

    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def calibrate(device) -> Session:
    """An event pair around the delay kernel: cycles of ``torch.cuda._sleep`` per millisecond, or -- where that does not hold
    the queue on this runtime -- element-wise kernels of a chain per millisecond.  This measures the hardware, not the library."""
    import torch

    s = Session()
    with torch.cuda.device(device):
        torch.cuda._sleep(1000)  # (loads the kernel)
        small, large = 2_000_000, 20_000_000
        t_small, t_large = _elapsed(lambda: torch.cuda._sleep(small)), _elapsed(lambda: torch.cuda._sleep(large))
        rate = (large - small) / max(t_large - t_small, 1e-6)  # cycles per ms
        s.notes.append(f"torch.cuda._sleep: {small} cycles {t_small:.3f} ms, {large} cycles {t_large:.3f} ms")
        if t_large - t_small > 1.0 and _elapsed(lambda: torch.cuda._sleep(int(rate * 20.0))) > 10.0:
            s.kind, s.unit_per_ms = "torch.cuda._sleep cycles", rate
            s.delay = lambda ms: torch.cuda._sleep(int(rate * ms))
            return s
        x = torch.zeros(1 << 22, device=device)

        def chain(k):
            for _ in range(int(k)):
                x.add_(1.0)

        chain(8)
        per_ms = 256 / max(_elapsed(lambda: chain(256)), 1e-6)
        s.notes.append("torch.cuda._sleep did not hold the queue: a chain of element-wise kernels instead")
        s.kind, s.unit_per_ms = "element-wise kernels of 4 Mi floats", per_ms
        s.delay = lambda ms: chain(max(per_ms * ms, 1.0))
    return s


def _probe_sees_decoy(session: Session, device, S, other, ms: float) -> Tuple[bool, bool]:
    """Torch operations only: behind a delay on S an input receives its true values late; ``input.clone()`` on ``other`` runs
    meanwhile -> (it saw the decoy, S was still busy when it had finished)."""
    import torch

    true = torch.arange(4096, dtype=torch.float32, device=device)
    decoy = -true - 1.0
    inp = decoy.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        session.delay(ms)
        inp.copy_(true)
    with torch.cuda.stream(other):
        probe = inp.clone()
        other.synchronize()
    held = not S.query()
    S.synchronize()
    assert torch.equal(inp, true)
    return torch.equal(probe, decoy), held


def choose_streams(session: Session, device, tries: int = 24) -> None:
    """``session.S`` and ``session.S2``: pool streams that this runtime does not serialise behind the default stream or behind
    each other.  A process has a few hardware queues (four here) and many streams; which streams share one is the runtime's
    business (it was not round robin over the order of creation where this was written), and two streams that share one see each
    other's work in order -- a launch that strayed from one to the other would return the right bits.  So the streams are
    screened with the positive control's own probe, and the control below then holds the chosen ones to it.
    The price: S is one handle for the whole session, so a library that cached a non-default stream handle from an earlier
    case's S and launched on it later would go unseen here (each case's recording wrappers still see what the Python layer
    hands over)."""
    import torch

    default = torch.cuda.default_stream(device)
    chosen = []
    for _ in range(tries):
        c = torch.cuda.Stream(device)
        if all(_probe_sees_decoy(session, device, c, o, 10.0)[0] and _probe_sees_decoy(session, device, o, c, 10.0)[0]
               for o in (default, *chosen)):
            chosen.append(c)
            if len(chosen) == 2:
                break
        else:
            session.notes.append(f"pool stream {c.cuda_stream:#x} shares a hardware queue with the default stream or with S: not used")
    session.S, session.S2 = (chosen + [None, None])[:2]


BLIND = ("the harness is blind on this machine: a clone on {other} observed the values that {S} copies in behind its delay, so "
         "{other} was serialised behind {S} (both mapped to one hardware queue, say) and a launch on the wrong stream could not "
         "be told from a right one")


def positive_control(session: Session, device) -> None:
    """The harness can see: with the cases' own delay and late ``copy_`` on S, ``probe = input.clone()`` on the DEFAULT stream
    must observe the decoy, and so must one on the second stream S2 (and on the default stream with S2 delayed: the side-stream
    cases and the two-renderer test issue there).  A probe that observes the true values means that stream was serialised
    behind the delayed one, and every case would pass whatever the library did."""
    import torch

    assert session.S is not None and session.S2 is not None, BLIND.format(
        other="the default stream (or every second pool stream)", S="every pool stream that was tried")
    default = torch.cuda.default_stream(device)
    for S, other, what in ((session.S, default, ("stream S", "the default stream")),
                           (session.S, session.S2, ("stream S", "the second pool stream S2")),
                           (session.S2, default, ("stream S2", "the default stream"))):
        saw_decoy, held = _probe_sees_decoy(session, device, S, other, DELAY_MS_MIN)
        assert held, f"positive control: the delay of {DELAY_MS_MIN} ms did not hold {what[0]} while {what[1]} ran"
        assert saw_decoy, BLIND.format(S=what[0], other=what[1])


SENTINEL = {"f": 12345.0, "i": -7, "u": 7}


def _snapshot(out: dict) -> dict:
    return {k: v.clone() for k, v in out.items()}


def _bytes(run: Run, snap: dict) -> dict:
    res = {}
    for k, v in snap.items():
        a = v.cpu().numpy()
        if k in run.canon:
            a = run.canon[k](a)
        res[k] = np.ascontiguousarray(a).tobytes()
    return res


def _warm_up(run: Run):
    import torch

    out = run.call()
    for k, v in out.items():  # outputs the object owns start from a sentinel: a call that left one alone shows
        if not k.startswith("state:") and v.numel():
            v.fill_(SENTINEL["f" if v.dtype.is_floating_point else "u" if v.dtype == torch.uint8 else "i"])


def baseline(case: Case, device) -> Tuple[dict, float]:
    """The default-stream run: warm-up on the decoys, the true inputs, the call -> (output bytes, host ms of the call)."""
    import torch

    run = case.build(device)
    _warm_up(run)
    for cur, true, _ in run.inputs.values():
        cur.copy_(true)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run.call()
    host_ms = (time.perf_counter() - t0) * 1e3
    snap = _snapshot(out)
    torch.cuda.synchronize()
    want = _bytes(run, snap)
    if run.check is not None:
        run.check()
    return want, host_ms


def delay_for(case: Case, host_ms: float, session: Session) -> float:
    delay_ms = min(DELAY_MS_MAX, max(DELAY_MS_MIN, DELAY_FACTOR * host_ms))
    if not case.synchronising:
        session.host_ms[case.name] = host_ms
        assert DELAY_FACTOR * host_ms <= DELAY_MS_MAX, (
            f"{case.name}: the Python call took {host_ms:.2f} ms of host time; no delay up to {DELAY_MS_MAX} ms is "
            f"{DELAY_FACTOR} x that")
    session.delay_ms[case.name] = delay_ms
    return delay_ms


def late_call(run: Run, S) -> Tuple[dict, bool]:
    """On the current stream S, which a delay kernel holds: the true inputs, the call, the snapshot, the decoys again
    -> (snapshot, whether S was still busy when the call returned)."""
    for cur, true, _ in run.inputs.values():
        cur.copy_(true, non_blocking=True)
    out = run.call()
    held = not S.query()
    snap = _snapshot(out)
    for cur, _, decoy in run.inputs.values():
        cur.copy_(decoy, non_blocking=True)
    return snap, held


def compare(case: Case, run: Run, snap: dict, want: dict, held: bool, delay_ms: float) -> None:
    got = _bytes(run, snap)
    if not case.synchronising:
        assert held, (f"{case.name}: stream S had drained when the call returned -- the delay of {delay_ms:.0f} ms did not "
                      f"hold, or the call waited for the stream although nothing says it does")
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (f"{case.name}: on a stream whose inputs arrive late, {differ} differ from the default-stream run "
                        f"bit for bit -- some launch, memset or copy of {case.covers} did not wait for its stream")


_SECOND = [None]


class second_stream:
    """While a delayed run is built: the stream a case takes as its own second stream (``a_second_stream``)."""

    def __init__(self, stream):
        self.stream = stream

    def __enter__(self):
        _SECOND[0] = self.stream

    def __exit__(self, *exc):
        _SECOND[0] = None


def a_second_stream(device):
    """A case's second stream: the session's S2 inside a delayed run (screened against S), any pool stream in a baseline."""
    import torch

    return _SECOND[0] if _SECOND[0] is not None else torch.cuda.Stream(device)


def run_case(case: Case, device, session: Session, allowed: Optional[set] = None) -> None:
    """Baseline and delayed run of ``case``; asserts the delay held and the bytes agree.  ``allowed`` (a set the caller's
    recording wrappers look at) holds the stream handles the delayed run may be issued on while it is being issued."""
    import torch

    t_wall = time.perf_counter()
    allowed = set() if allowed is None else allowed
    with torch.cuda.device(device):
        want, host_ms = baseline(case, device)
        delay_ms = delay_for(case, host_ms, session)
        S = session.S
        try:
            with torch.cuda.stream(S), second_stream(session.S2):
                allowed.add(S.cuda_stream)
                run = case.build(device)
                allowed.update(s.cuda_stream for s in run.extra_streams)
                _warm_up(run)
                torch.cuda.synchronize()
                session.delay(delay_ms)
                snap, held = late_call(run, S)
                S.synchronize()
        finally:
            allowed.clear()
        torch.cuda.synchronize()
        compare(case, run, snap, want, held, delay_ms)
        del run, snap
    session.wall_s[case.name] = time.perf_counter() - t_wall


def write_report(session: Session, cases: List[Case], path: str) -> None:
    lines = [f"delay kernel: {session.kind}, {session.unit_per_ms:.1f} per ms", *session.notes,
             f"delay per case: max({DELAY_MS_MIN:.0f} ms, {DELAY_FACTOR:.0f} x the host time of its call), at most "
             f"{DELAY_MS_MAX:.0f} ms", ""]
    done = [c for c in cases if c.name in session.wall_s]
    slow = max((session.host_ms.get(c.name, 0.0) for c in done), default=0.0)
    lines += [f"cases run: {len(done)}; slowest asynchronous call {slow:.3f} ms of host time; the tier's wall time "
              f"{sum(session.wall_s.values()):.1f} s", "", "case, host ms of the call, delay ms, wall s"]
    for c in done:
        h = session.host_ms.get(c.name)
        lines.append(f"  {c.name}: {'(synchronising)' if c.synchronising else '-' if h is None else f'{h:.3f}'}, "
                     f"{session.delay_ms[c.name]:.0f}, "
                     f"{session.wall_s[c.name]:.2f}")
    lines += ["", "synchronising cases (exempt from the delay-held assertion; their bits are compared all the same)"]
    lines += [f"  {c.name}: {c.synchronising}" for c in cases if c.synchronising]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------- shared data (host)
W0, H0 = 96, 64      # the smaller frame
W1, H1 = 160, 112    # the larger one
MAX_PAIRS = 1 << 17  # several times what 6,000 Gaussians list at these sizes (17,099 pairs): no case may overflow (each checks)


@functools.lru_cache(maxsize=None)
def _scene(n, W, H, seed, sh=0):
    from gs_scene import make_scene

    return make_scene(n, W, H, seed=seed, use_sh=bool(sh), sh_degree=sh or 2)


def _camera(W, H, yaw=2.0, pp=False):
    from gs_scene import make_camera

    cam = make_camera(W, H, yaw_deg=yaw)
    cam.tran = np.array([0.05, -0.02, 0.1], np.float32)
    if pp:
        cam.cx, cam.cy = W / 2 + 5.25, H / 2 - 3.5
    return cam


@functools.lru_cache(maxsize=None)
def _oracle_frame(n, W, H, seed, sh=0):
    from gs_testutil import OracleFrame

    return OracleFrame(_scene(n, W, H, seed, sh), _camera(W, H, 3.0))


def _rng(seed):
    return np.random.default_rng(seed)


def _roll(a):
    """A valid decoy of a sorted, per-pair array: the same rows in another place."""
    return np.roll(a, max(len(a) // 2, 1), axis=0)


def _scene_inputs(run: Run, n, W, H, sh=0, seeds=(11, 12)):
    true, decoy = _scene(n, W, H, seeds[0], sh), _scene(n, W, H, seeds[1], sh)
    return [run.input(k, getattr(true, k), getattr(decoy, k)) for k in ("pos", "quat", "scale", "opa", "rgb")]


def _image_input(run: Run, name, shape, seeds, lo=0.0, hi=1.0):
    return run.input(name, *(_rng(s).uniform(lo, hi, shape).astype(np.float32) for s in seeds))


def _normal_input(run: Run, name, shape, seeds, scale=1.0):
    return run.input(name, *((_rng(s).standard_normal(shape) * scale).astype(np.float32) for s in seeds))


def _zeros(device, *shape, dtype=None):
    import torch

    return torch.zeros(*shape, dtype=dtype or torch.float32, device=device)


def _no_overflow(r):
    def check():
        st = r.stats()
        assert st.overflow == 0 and st.pairs > 0, f"the case's frame overflowed or is empty: {st}"
    return check


# ---------------------------------------------------------------------------------------------------- reference API
def _ref_world2camera(device):
    import gaussian

    run = Run(device)
    pos = _normal_input(run, "pos", (1001, 3), (1, 2))
    gout = _normal_input(run, "grad_out", (1001, 3), (3, 4))
    rot = run.input("rot", _camera(W0, H0, 3.0).rot, _camera(W0, H0, -8.0).rot)
    tran = run.input("tran", np.array([0.05, -0.02, 4.0], np.float32), np.array([-0.5, 0.3, 6.0], np.float32))
    res, gi, jac = _zeros(device, 1001, 3), _zeros(device, 1001, 3), _zeros(device, 1001, 3, 3)

    def call():
        gaussian.world2camera(pos, rot, tran, res)
        gaussian.jacobian(res, jac)
        gaussian.world2camera_backward(gout, rot, gi)
        return {"res": res, "jacobian": jac, "grad_inp": gi}

    run.call = call
    return run


def _ref_global_culling(device):
    import gaussian
    import torch
    from gs_testutil import activate, frame_scalars

    run = Run(device)
    n = 5000
    sc = [_scene(n, W1, H1, s) for s in (11, 12)]
    act = [activate(s) for s in sc]
    cams = [_camera(W1, H1, 3.0), _camera(W1, H1, -5.0)]
    _, hw, hh, _ = frame_scalars(cams[0])
    pos = run.input("pos", sc[0].pos, sc[1].pos)
    qn = run.input("quat", act[0][0], act[1][0])
    sn = run.input("scale", act[0][1], act[1][1])
    rot = run.input("rot", cams[0].rot, cams[1].rot)
    tran = run.input("tran", cams[0].tran, cams[1].tran + np.float32(0.2))
    gop = _normal_input(run, "gradout_pos", (n, 3), (5, 6))
    goc = _normal_input(run, "gradout_cov", (n, 2, 2), (7, 8))
    res_pos, res_cov = _zeros(device, n, 3), _zeros(device, n, 2, 2)
    mask = _zeros(device, n, dtype=torch.long)
    grads = [_zeros(device, n, k) for k in (3, 4, 3)]

    def call():
        for t in (res_pos, res_cov, mask, *grads):  # the caller pre-zeroes (renderer.py): culled rows are left untouched
            t.zero_()
        gaussian.global_culling(pos, qn, sn, rot, tran, res_pos, res_cov, mask, cams[0].near, hw, hh)
        gaussian.global_culling_backward(pos, qn, sn, rot, tran, gop, goc, mask, *grads)
        return {"res_pos": res_pos, "res_cov": res_cov, "mask": mask, "grad_pos": grads[0], "grad_quat": grads[1],
                "grad_scale": grads[2]}

    run.call = call
    return run


@functools.lru_cache(maxsize=None)
def _tile_lists(method):
    """Projected Gaussians of the small frame and the oracle's tile lists for them: (grid, pos_i, cov, thresh, counts, lists)."""
    import oracle

    of = _oracle_frame(3000, W1, H1, 7)
    keep = of.mask.astype(bool)
    grid, pos_i, cov = of.grid, of.pos_i[keep], of.cov.reshape(-1, 4)[keep]
    thresh = 0.05 if method else (grid.tile_geo_length_x / 0.3) ** 2
    top, bottom, left, right = grid.tile_edges()
    maxp = pos_i.shape[0]  # no tile can overflow: the SET a tile keeps is then defined (its order is atomic order)
    n_ref, list_ref = oracle.calc_tile_list(pos_i, cov, maxp, thresh, method, grid.tile_geo_length_x, grid.tile_geo_length_y,
                                            grid.n_tile_x, grid.n_tile_y, grid.leftmost, grid.topmost, top, bottom, left, right)
    return grid, pos_i, cov, thresh, n_ref, list_ref


def _ref_calc_tile_list(method):
    def build(device):
        import gaussian
        import torch

        run = Run(device)
        grid, pos_i, cov, thresh, n_ref, _ = _tile_lists(method)
        maxp = int(n_ref.max()) + 1
        g3, ti = gaussian.Gaussian3ds(), gaussian.Tiles()
        g3.pos = run.input("pos", pos_i, _roll(pos_i))
        g3.cov = run.input("cov", cov.reshape(-1, 2, 2), _roll(cov.reshape(-1, 2, 2)))
        ti.top, ti.bottom, ti.left, ti.right = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in grid.tile_edges())
        count = _zeros(device, grid.n_tiles, dtype=torch.int32)
        lists = _zeros(device, grid.n_tiles, maxp, dtype=torch.int32)

        def call():
            count.zero_()  # "tile_n_point [T] int32 must be zeroed by the caller"
            lists.fill_(-1)
            gaussian.calc_tile_list(g3, ti, count, lists, thresh, method, grid.tile_geo_length_x, grid.tile_geo_length_y,
                                    grid.n_tile_x, grid.n_tile_y, grid.leftmost, grid.topmost)
            return {"tile_n_point": count, "tile_gaussian_list": lists}

        run.call = call
        run.canon["tile_gaussian_list"] = lambda a: np.sort(a, axis=1)  # a tile's entries arrive in atomic order
        return run

    return build


def _ref_gather(device):
    import gaussian
    import torch

    run = Run(device)
    grid, _, _, _, n_ref, list_ref = _tile_lists(2)
    maxp = int(n_ref.max()) + 1
    lists_true = np.where(np.arange(maxp)[None, :] < n_ref[:, None], list_ref[:, :maxp], 0).astype(np.int32)
    accum_true = np.concatenate([[0], np.cumsum(n_ref)]).astype(np.int32)
    M = int(accum_true[-1])
    accum = run.input("tile_n_point_accum", accum_true, np.zeros_like(accum_true))  # zeros: empty lists
    lists = run.input("tile_gaussian_list", lists_true, np.zeros_like(lists_true))
    gathered, tile_ids = _zeros(device, M, dtype=torch.int32), _zeros(device, M, dtype=torch.int32)

    def call():
        gaussian.gather_gaussians(accum, lists, gathered, tile_ids, maxp)
        return {"gathered_list": gathered, "tile_ids_for_points": tile_ids}

    run.call = call
    return run


def _ref_draw(sh, sigmoid, fast):
    def build(device):
        import gaussian
        import torch

        run = Run(device)
        of = _oracle_frame(6000, W0, H0, 2, 2 if sh else 0)
        assert np.diff(of.accum).max() > 64  # one tile list longer than a bucket
        grid, rays = of.grid, of.rays
        cov = of.s_cov.reshape(-1, 2, 2)
        t = [run.input(k, a, _roll(a)) for k, a in (("pos", of.s_pos), ("rgb", of.s_rgb), ("opa", of.s_opa), ("cov", cov))]
        accum = run.input("tile_n_point_accum", of.accum.astype(np.int32), np.zeros_like(of.accum, dtype=np.int32))
        gout = _normal_input(run, "grad_output", of.padded.shape, (9, 10))
        rv = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device) if sh else None
              for v in (rays.rays_o, rays.lefttop, rays.dx, rays.dy)]
        res = _zeros(device, grid.padded_height, grid.padded_width, 3)
        grads = [torch.zeros_like(x) for x in t]

        def call():
            for x in (res, *grads):  # the caller pre-zeroes (renderer.py)
                x.zero_()
            gaussian.draw(*t, accum, res, grid.focal_x, grid.focal_y, False, sigmoid, fast, *rv, sh)
            gaussian.draw_backward(*t, accum, res, gout, *grads, grid.focal_x, grid.focal_y, False, sigmoid, fast, *rv, sh)
            return {"image": res, "grad_pos": grads[0], "grad_rgb": grads[1], "grad_opa": grads[2], "grad_cov": grads[3]}

        run.call = call
        return run

    return build


SORT_ONE_TRIP = 2048 * 256  # radix_sort.hip: pairs of one trip of the row scan (tests/test_gpu_step_regimes.py)


def _sort(n, bits):
    def build(device):
        import torch
        from gaussian import _lib

        run = Run(device)
        cap = n + 1000

        def keys_of(seed):
            rng = _rng(seed)
            tiles = rng.integers(0, 700, cap).astype(np.uint64)
            depth = rng.integers(0, 40, cap).astype(np.uint64) * np.uint64(0x01000193) % np.uint64(1 << 32)
            return ((tiles << np.uint64(32)) | depth).view(np.int64)

        keys = run.input("keys", keys_of(n + 11), keys_of(n + 12))
        count = run.input("count", np.array([n, 0], np.int32), np.zeros(2, np.int32))  # the count arrives late as well
        vals = torch.arange(cap, dtype=torch.int32, device=device)
        k0, v0, k1, v1 = torch.empty_like(keys), torch.empty_like(vals), torch.empty_like(keys), torch.empty_like(vals)
        tmp = torch.zeros(_lib.gs_sort_pairs_tmp_bytes(cap), dtype=torch.uint8, device=device)
        in1 = C.c_int(-1)

        def call():
            k0.copy_(keys)  # (the sort destroys buffer 0)
            v0.copy_(vals)
            k1.zero_()
            v1.zero_()
            stream = torch.cuda.current_stream().cuda_stream
            head = (k0.data_ptr(), v0.data_ptr(), k1.data_ptr(), v1.data_ptr(), count.data_ptr(), cap)
            tail = (tmp.data_ptr(), tmp.numel(), C.byref(in1), stream)
            if bits:
                _lib.check(_lib.gs_sort_pairs_bits(*head, 32, 42, *tail), "gs_sort_pairs_bits")
            else:
                _lib.check(_lib.gs_sort_pairs(*head, 42, *tail), "gs_sort_pairs")
            ks, vs = (k1, v1) if in1.value else (k0, v0)
            return {"keys": ks[:n], "vals": vs[:n]}

        run.call = call
        return run

    return build


# ---------------------------------------------------------------------------------------------------- frame path
def _renderer(device, training, **kw):
    from gs_frame import FrameRenderer

    kw = {"auto_grow": False, "occlusion_cull": False, "scene_pack": False, "force_strips": True, **kw}
    return FrameRenderer(device, max_pairs=MAX_PAIRS, training=training, **kw)


def _frame_inference(W, H, n, sh=0, aux=False, pp=False, frames=1, **kw):
    """``frames`` consecutive inference frames of one scene and camera -> every frame's image (and maps)."""
    def build(device):
        run = Run(device)
        params = _scene_inputs(run, n, W, H, sh)
        cam = _camera(W, H, pp=pp)
        r = _renderer(device, False, **kw)

        flags = []

        def call():
            out = {}
            del flags[:]
            for k in range(frames):
                res = r.forward(*params, cam, aux=aux)
                flags.append(int(r._frame.flags))
                out[f"image{k}"] = res[0]
                if aux:
                    out[f"depth{k}"], out[f"alpha{k}"] = res[2], res[3]
            return out

        run.call = call
        run.check = _no_overflow(r)
        if kw.get("scene_pack", False) is None:  # GS_FRAME_SCENE_PACK: built in front of the second frame, read by the third
            run.check = lambda: (_no_overflow(r)(), _assert(flags[-1] & 8192, "the last frame read no scene pack"))
        if kw.get("occlusion_cull"):  # GS_FRAME_OCCLUSION_CULL (which frames carry it follows the renderer's own probes)
            run.check = lambda: (_no_overflow(r)(), _assert(any(f & 256 for f in flags), "no frame of the call was culled"))
        return run

    return build


def _assert(cond, what):
    assert cond, what


def _frame_cull_repeat(device):
    """Three forwards at one pose inside the call: an unculled frame, an occlusion-culled frame from the scene pack built in
    front of it, then that frame again with GS_FRAME_CULL_REPEAT set by hand on a copy of its descriptor (the renderer's own
    licence needs counters that have reached the host; the promise is made here as tests/test_gpu_raster_compact.py makes it:
    the same descriptor, the same scene bytes, and -- ``check`` -- the culled frame of exactly these inputs ran past nothing)."""
    import torch
    from gaussian import _lib
    from gs_frame import FrameRenderer

    run = Run(device)
    W, H = W0, H0
    params = _scene_inputs(run, 5000, W, H)
    cam = _camera(W, H)
    r = FrameRenderer(device, max_pairs=MAX_PAIRS, auto_grow=False, force_strips=True, cull_second_pass="always")
    host = [torch.zeros(_lib.GS_STATS_TAGGED_N, dtype=torch.int64).pin_memory() for _ in range(2)]
    flags = []

    def call():
        s = torch.cuda.current_stream().cuda_stream
        del flags[:]
        r._cut_key = None  # (no cut table yet: the first frame of the call is unculled, as a fresh renderer's)
        images = []
        for k in range(2):
            r._cull_off_until = 0  # (the adaptive policy kept out of the way)
            images.append(r.forward(*params, cam)[0])
            flags.append(int(r._frame.flags))
        _lib.call("gs_frame_stats_tagged_async", C.byref(r._frame), 78, host[0].data_ptr(), s)
        f = _lib.GsFrameDP()
        C.memmove(C.byref(f), C.byref(r._frame), C.sizeof(_lib.GsFrameDP))
        f.flags |= _lib.GS_FRAME_CULL_REPEAT
        image = torch.full((H, W, 3), -7.0, device=device)
        f.image = image.data_ptr()
        _lib.call("gs_frame_forward", C.byref(f), s)
        _lib.call("gs_frame_stats_tagged_async", C.byref(f), 79, host[1].data_ptr(), s)
        back = [h.to(device, non_blocking=True) for h in host]
        pick = lambda b: torch.cat([b[:3], b[10:12]])  # noqa: E731 (visible, pairs, overflow, ran past, tag)
        return {"image0": images[0], "image1": images[1], "image_repeat": image, "counters_culled": pick(back[0]),
                "counters_repeat": pick(back[1])}

    def check():
        want = _lib.GS_FRAME_OCCLUSION_CULL | _lib.GS_FRAME_SCENE_PACK
        assert not flags[0] & want and flags[1] & want == want, [hex(x) for x in flags]
        for h, tag in zip(host, (78, 79)):
            v = h.tolist()
            assert int(v[11]) & 0xffffffff == tag and v[1] > 0 and v[2] == 0 and v[10] == 0, (tag, v)

    run.call = call
    run.check = check
    return run


def _frame_device_pose(device):
    """A training forward that reads its pose from device memory (GS_FRAME_DEVICE_POSE), the 12 floats among the late inputs,
    and the pose-only backward, the one backward such a frame has."""
    run = Run(device)
    W, H = W0, H0
    params = _scene_inputs(run, 5000, W, H)
    gi = _normal_input(run, "grad_image", (H, W, 3), (21, 22))
    cam, other = _camera(W, H), _camera(W, H, yaw=-4.0)
    pose = run.input("pose_dev", *(np.concatenate([c.rot.reshape(9), c.tran]).astype(np.float32) for c in (cam, other)))
    r = _renderer(device, True)
    grad_pose = (_zeros(device, 3, 3), _zeros(device, 3))

    def call():
        image, padded = r.forward(*params, cam, training=True, pose_dev=pose)
        r.backward_pose(gi, grad_pose, 0)
        return {"image": image, "padded": padded, "grad_rot": grad_pose[0], "grad_tran": grad_pose[1]}

    run.call = call
    run.check = _no_overflow(r)
    return run


def _frame_counters(device):
    """An inference frame and the four counter copies behind it, read through pinned memory."""
    import torch
    from gaussian import _lib

    run = Run(device)
    params = _scene_inputs(run, 5000, W0, H0)
    cam = _camera(W0, H0)
    r = _renderer(device, False)
    host = [torch.zeros(k, dtype=torch.int64).pin_memory() for k in (4, 1, 1, _lib.GS_STATS_TAGGED_N)]

    def call():
        image, _ = r.forward(*params, cam)
        f, s = C.byref(r._frame), torch.cuda.current_stream().cuda_stream
        _lib.call("gs_frame_stats_async", f, host[0].data_ptr(), s)
        _lib.call("gs_frame_longest_list_async", f, host[1].data_ptr(), s)
        _lib.call("gs_frame_cull_fallback_async", f, host[2].data_ptr(), s)
        _lib.call("gs_frame_stats_tagged_async", f, 77, host[3].data_ptr(), s)
        back = [h.to(device, non_blocking=True) for h in host]  # (stream-ordered behind the copies that fill the host side)
        return {"image": image, "visible_pairs_overflow": back[0][:3], "longest": back[1], "ran_past": back[2],
                "tagged": torch.cat([back[3][:3], back[3][9:12]])}

    run.call = call
    run.check = _no_overflow(r)
    return run


def _frame_stats(device):
    run = Run(device)
    params = _scene_inputs(run, 5000, W0, H0)
    cam = _camera(W0, H0)
    r = _renderer(device, False)

    def call():
        import torch

        image, _ = r.forward(*params, cam)
        st = r.stats()
        return {"image": image, "stats": torch.tensor([st.visible, st.pairs, st.overflow], device=device)}

    run.call = call
    return run


def _frame_profile(device):
    """gs_frame_forward_profile and gs_frame_backward_profile: the frame's work between hipEvents, the same results."""
    import torch
    from gaussian import _lib

    run = Run(device)
    W, H, n = W0, H0, 5000
    params = _scene_inputs(run, n, W, H)
    gi = _normal_input(run, "grad_image", (H, W, 3), (21, 22))
    cam = _camera(W, H)
    r = _renderer(device, True, bwd_rows=False)
    out = [torch.zeros_like(t) for t in params]
    ms = (C.c_float * 3)()

    def call():
        r.profile_forward(*params, cam, training=True)
        _lib.call("gs_frame_backward_profile", C.byref(r._frame), gi.data_ptr(), *(t.data_ptr() for t in out), ms,
                  torch.cuda.current_stream().cuda_stream)
        return {"image": r._keep[5], "padded": r._keep[6], **{f"grad{k}": t for k, t in enumerate(out)}}

    run.call = call
    run.check = _no_overflow(r)
    return run


def _grad_inputs(run, W, H, aux, image=True):
    gi = _normal_input(run, "grad_image", (H, W, 3), (21, 22)) if image else None
    gd = _normal_input(run, "grad_depth", (H, W), (23, 24), 0.1) if aux else None
    ga = _normal_input(run, "grad_alpha", (H, W), (25, 26)) if aux else None
    return gi, gd, ga


def _frame_training(W, H, n, sh=0, aux=False, mode="one", pp=False, seeds=(11, 12), **kw):
    """A training forward and its backward.  ``mode``: "one" call; "parts" (raster, geometry, colour); "slices" (raster, then
    the per-Gaussian sums in two ranges); "begin" (the forward issued in slice ranges behind a frame of another view)."""
    def build(device):
        import torch
        from gaussian import _lib

        run = Run(device)
        params = _scene_inputs(run, n, W, H, sh, seeds)
        gi, gd, ga = _grad_inputs(run, W, H, aux)
        cam, other = _camera(W, H, pp=pp), _camera(W, H, yaw=-6.0, pp=pp)
        r = _renderer(device, True, **kw)
        out = [torch.zeros_like(t) for t in params]

        def call():
            if mode == "begin":
                r.forward(*params, other)  # (a slice that nobody projected would hold that view's records)
                assert r.forward_begin(*params, cam, 0, 3) is True, "the renderer declined to issue the frame in slice ranges"
                assert r.forward_begin(*params, cam, 3, 1 << 30)
                res = r.forward_finish()
            else:
                res = r.forward(*params, cam, aux=aux)
            kwa = dict(grad_depth=gd, grad_alpha=ga) if aux else {}
            if mode == "parts":
                r.backward(gi, out=out, part=_lib.GS_BWD_RASTER, **kwa)
                r.backward(None, out=out, part=_lib.GS_BWD_COLOR)
                r.backward(None, out=out, part=_lib.GS_BWD_GEOMETRY)
            elif mode == "slices":
                r.backward(gi, out=out, part=_lib.GS_BWD_RASTER, **kwa)
                cut = 256 * ((n // 256) // 2)
                r.backward_slice(out, cut, n)
                r.backward_slice(out, 0, cut)
            else:
                r.backward(gi, out=out, **kwa)
            res_d = {"image": res[0], "padded": res[1], **{f"grad{k}": t for k, t in enumerate(out)}}
            if aux:
                res_d["depth"], res_d["alpha"] = res[2], res[3]
            return res_d

        run.call = call
        run.check = _no_overflow(r)
        return run

    return build


def _flat_scene(run: Run, n, W, H, seeds=(11, 12)):
    """The scene as a gs_dp.FlatGaussianParams whose flat buffer is the (one) late input -> (flat, its five views)."""
    import torch
    from gs_dp import FlatGaussianParams

    sc = [_scene(n, W, H, s) for s in seeds]
    flats = []
    for s in sc:
        flats.append(FlatGaussianParams([torch.from_numpy(getattr(s, k)).to(run.device)
                                         for k in ("pos", "quat", "scale", "opa", "rgb")]))
    flat = flats[1]
    run.input("state:flat_param", flats[0].flat_param.cpu().numpy(), flats[1].flat_param.cpu().numpy(), into=flat.flat_param)
    return flat, flat.params


def _frame_fused_adam(W, H, n, kind, seeds=(11, 12)):
    """forward + the fused backward and Adam step: "plain", "aux" (grad_image None: the library's zero image) or "pose"."""
    def build(device):
        from gs_train import FusedAdam

        run = Run(device)
        flat, params = _flat_scene(run, n, W, H, seeds)
        aux = kind == "aux"
        gi, gd, ga = _grad_inputs(run, W, H, aux, image=not aux)
        cam = _camera(W, H)
        r = _renderer(device, True)
        opt = FusedAdam(flat, [1e-3, 2e-3, 3e-3, 4e-3, 5e-3], grad_stat="max")
        grad_pose = (_zeros(device, 3, 3), _zeros(device, 3)) if kind == "pose" else None

        def call():
            res = r.forward(*params, cam, aux=aux)
            r.backward_adam(gi, opt.fused_descriptor(), grad_depth=gd, grad_alpha=ga, grad_pose=grad_pose)
            out = {"image": res[0], "state:params": flat.flat_param, "state:exp_avg": opt.exp_avg,
                   "state:exp_avg_sq": opt.exp_avg_sq, "state:grad_stat": opt.accum_grad}
            if grad_pose is not None:
                out["grad_rot"], out["grad_tran"] = grad_pose
            return out

        run.call = call
        run.check = _no_overflow(r)
        return run

    return build


def _frame_pose_only(device):
    run = Run(device)
    W, H, n = W0, H0, 5000
    params = _scene_inputs(run, n, W, H)
    gi, gd, ga = _grad_inputs(run, W, H, True)
    cam = _camera(W, H)
    r = _renderer(device, True)
    grad_pose = (_zeros(device, 3, 3), _zeros(device, 3))

    def call():
        res = r.forward(*params, cam, aux=True)
        r.backward_pose(gi, grad_pose, 0, grad_depth=gd, grad_alpha=ga)
        return {"image": res[0], "depth": res[2], "alpha": res[3], "grad_rot": grad_pose[0], "grad_tran": grad_pose[1]}

    run.call = call
    run.check = _no_overflow(r)
    return run


def _frame_contrib(device):
    run = Run(device)
    params = _scene_inputs(run, 5000, W0, H0)
    cam = _camera(W0, H0)
    r = _renderer(device, True)

    def call():
        image, _ = r.forward(*params, cam)
        return {"image": image, "rows": r.contributions().rows}

    run.call = call
    run.check = _no_overflow(r)
    return run


# The library's own side stream.  include/gs_abi.h, gs_frame_forward: "With f->training AND f->async the zero-fill of the
# per-pair gradient rows and the backward's bucket list are issued on the handle's side stream, which waits for the frame's last
# kernel [...]; gs_frame_backward -- from any host thread -- and the next gs_frame_forward with the same handle wait for that
# stream's event."  FrameRenderer always carries a handle, so every training case above crosses the side stream on S; the three
# cases below put the caller's loss in between, hand the backward to ANOTHER stream behind ``S2.wait_stream(S)`` (the sentence
# above is what makes that legal: the backward's stream, not the forward's, is made to wait for the handle's event), and
# release and regrow the workspace there (gs_frame_async_wait: "make `stream` wait for side-stream work that may still be
# writing into the workspace of the handle's last training forward").
def _side_stream(kind):
    def build(device):
        import torch
        from gs_train import ImageLoss

        run = Run(device)
        W, H, n = W0, H0, 5000
        params = _scene_inputs(run, n, W, H)
        target = _image_input(run, "target", (H, W, 3), (31, 32))
        cam = _camera(W, H)
        r = _renderer(device, True)
        if kind == "release":
            r.max_pairs = MAX_PAIRS >> 2  # (doubled by the warm-up and again by the call)
        loss = ImageLoss(H, W, device=device)
        S2 = a_second_stream(device) if kind != "same" else None
        if S2 is not None:
            run.extra_streams.append(S2)
            for t in (*params, target, loss.grad, loss.values):
                t.record_stream(S2)

        def call():
            S = torch.cuda.current_stream()
            image, padded = r.forward(*params, cam)
            if kind == "same":
                grads = r.backward(loss(image, target))
                return {"image": image, "loss_grad": loss.grad, "loss_values": loss.values,
                        **{f"grad{k}": t for k, t in enumerate(grads)}}
            S2.wait_stream(S)
            with torch.cuda.stream(S2):
                if kind == "backward":
                    grads = r.backward(loss(image, target))
                    out = {"image": image, "loss_grad": loss.grad, "loss_values": loss.values,
                           **{f"grad{k}": t for k, t in enumerate(grads)}}
                else:  # the frame gets no backward: its workspace is released and a larger one takes its place
                    r._release_workspace()
                    r.max_pairs *= 2  # (a growth of max_pairs: the next forward allocates, behind another gs_frame_async_wait)
                    image2, padded2 = r.forward(*params, cam)
                    grads = r.backward(loss(image2, target))
                    out = {"image": image, "image2": image2, **{f"grad{k}": t for k, t in enumerate(grads)}}
                for t in out.values():
                    t.record_stream(S)
            S.wait_stream(S2)  # (the snapshot is taken on S)
            return out

        run.call = call
        run.check = _no_overflow(r)
        return run

    return build


# ---------------------------------------------------------------------------------------------------- training-step kernels
MAP_NAMES = ("image", "depth", "alpha", "target_image", "target_range")


def _maps(run, H, W, only=MAP_NAMES):
    """The maps of a tracking loss named in ``only``, registered as late inputs, in MAP_NAMES order (None for the others):
    alpha on both sides of 0.5, depth = alpha z, a range map with holes."""
    def host(seed):
        rng = _rng(seed)
        alpha = rng.uniform(0.2, 1.0, (H, W)).astype(np.float32)
        z = rng.uniform(1.0, 4.0, (H, W)).astype(np.float32)
        rng_map = (z + rng.normal(0, 0.05, (H, W))).astype(np.float32)
        rng_map[rng.uniform(size=(H, W)) < 0.1] = 0.0  # no measurement
        return (rng.uniform(0, 1, (H, W, 3)).astype(np.float32), (alpha * z).astype(np.float32), alpha,
                rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng_map)

    return [run.input(k, a, b) if k in only else None for k, a, b in zip(MAP_NAMES, host(41), host(42))]


def _image_loss(H, W, weighted=False):
    def build(device):
        from gs_train import ImageLoss, WeightedImageLoss

        run = Run(device)
        pred = _image_input(run, "pred", (H, W, 3), (33, 34))
        target = _image_input(run, "target", (H, W, 3), (35, 36))
        if weighted:
            w_true = (_rng(37).uniform(size=(H, W)) > 0.3).astype(np.float32)
            weight = run.input("weight", w_true, (_rng(38).uniform(size=(H, W)) > 0.6).astype(np.float32))
            sums = (float(w_true.sum(dtype=np.float64)), float(w_true[5:H - 5, 5:W - 5].sum(dtype=np.float64)))
            loss = WeightedImageLoss(H, W, device=device)
        else:
            loss = ImageLoss(H, W, device=device)

        def call():
            loss(pred, target, weight, *sums) if weighted else loss(pred, target)
            return {"grad": loss.grad, "values": loss.values}

        run.call = call
        return run

    return build


def _depth_loss(device):
    from gs_train import DepthLoss

    run = Run(device)
    H, W = 31, 33
    _, depth, alpha, _, target = _maps(run, H, W, ("depth", "alpha", "target_range"))
    loss = DepthLoss(H, W, device=device)

    def call():
        loss(depth, alpha, target, 1.0 / (H * W))
        return {"grad_depth": loss.grad_depth, "grad_alpha": loss.grad_alpha, "values": loss.values}

    run.call = call
    return run


def _track_loss(kind):
    def build(device):
        from gs_train import GatedTrackLoss, GateMask, TrackLoss

        run = Run(device)
        H, W = 53, 83
        maps = _maps(run, H, W)
        if kind == "plain":
            loss = TrackLoss(H, W, device=device)
        elif kind == "gated":
            loss = GatedTrackLoss(H, W, depth_gate_k=2.5, color_gate_k=3.0, device=device)
        else:
            loss = GateMask(H, W, depth_gate_k=2.5, color_gate_k=3.0, device=device)

        def call():
            if kind == "mask":
                loss(*maps)
                return {"range": loss.range, "weight": loss.weight, "values": loss.values}
            loss(*maps, 1.0 / (H * W))
            return {"grad_image": loss.grad_image, "grad_depth": loss.grad_depth, "grad_alpha": loss.grad_alpha,
                    "values": loss.values}

        run.call = call
        return run

    return build


ADAM_GRID_CAP = 256 * 16 * 256 * 4   # adam.hip: elements of one launch without the stride loop (test_gpu_step_regimes.py)
ADAM_N = ADAM_GRID_CAP + 4_099
ADAM_ENDS = [7, 310, 311, 640, ADAM_N]  # test_adam_group_boundaries_inside_a_float4's table, its last group out to n
ADAM_LRS = [0.03, 0.02, 0.003, 0.004, 0.005]


@functools.lru_cache(maxsize=None)
def _adam_host(seed):
    return _rng(seed).standard_normal(ADAM_N, dtype=np.float32)


def _adam(kind, skip=None):
    """gs_adam_step / _range / _sharded / _multi over one flat array.  ``skip``: the value of the device skip flag, which arrives
    late like the parameters and the gradient (its decoy is the other value)."""
    def build(device):
        import torch
        from gaussian import _lib

        run = Run(device)
        n = ADAM_N
        p = run.input("state:param", _adam_host(51), _adam_host(52))
        g = run.input("grad", _adam_host(53), _adam_host(54))
        m, v = _zeros(device, n), _zeros(device, n)
        stat = _zeros(device, 3000)
        flag = run.input("skip_flag", np.array([skip], np.int64), np.array([1 - skip], np.int64)) if skip is not None else None
        ends, lrs = (C.c_int64 * 5)(*ADAM_ENDS), (C.c_float * 5)(*ADAM_LRS)
        step = [0]

        def call():
            step[0] += 1
            s = torch.cuda.current_stream().cuda_stream
            head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n)
            tail = (5, ends, lrs, 0.9, 0.99, 1e-8, step[0], stat.data_ptr(), 1_000_001, 1_003_001, 1)
            if kind == "one":
                _lib.call("gs_adam_step", *head, *tail, s)
            elif kind == "range":
                for lo, hi in ((0, 5), (5, 1_500_001), (1_500_001, n)):
                    _lib.call("gs_adam_step_range", *head, lo, hi, *tail, s)
            elif kind == "sharded":
                _lib.call("gs_adam_step_sharded", *head, 0, n, 0, *tail, flag.data_ptr(), s)
            else:
                los, his = (C.c_int64 * 3)(0, 308, 2_000_004), (C.c_int64 * 3)(308, 2_000_004, n)
                _lib.call("gs_adam_step_multi", *head, 3, los, his, los, *tail, flag.data_ptr(), 0.5, s)
            return {"state:param": p, "state:exp_avg": m, "state:exp_avg_sq": v, "state:grad_stat": stat}

        run.call = call
        return run

    return build


def _grad_stat(device):
    import torch
    from gaussian import _lib

    run = Run(device)
    n = 5003
    grad = _normal_input(run, "pos_grad", (n, 3), (55, 56))
    accum = _zeros(device, n, 3)

    def call():
        _lib.call("gs_grad_stat_update", grad.data_ptr(), accum.data_ptr(), accum.numel(), 1,
                  torch.cuda.current_stream().cuda_stream)
        return {"state:accum": accum}

    run.call = call
    return run


def _exposure(free):
    def build(device):
        from gs_exposure import Exposure

        run = Run(device)
        H, W = 31, 33
        image = _image_input(run, "image", (H, W, 3), (61, 62))
        grad = _normal_input(run, "state:grad", (H, W, 3), (63, 64))
        ex = Exposure(H, W, device, gain=(1.1, 0.9, 1.05), bias=(0.02, -0.01, 0.0))
        if free:
            ex.free(3e-2, 2e-2)

        def call():
            out = ex.apply(image)
            ex.backward(image, grad)  # (scales `grad` in place; free: one Adam step on the six numbers, on the device)
            res = {"compensated": out, "state:grad": grad, "grad_numbers": ex.grad, "state:numbers": ex.numbers}
            if free:
                res["state:adam"] = ex._fit.state
            return res

        run.call = call
        return run

    return build


def _pyramid(device):
    from gs_pyramid import Pyramid

    run = Run(device)
    H, W = 56, 88
    image, _, _, _, rng_map = _maps(run, H, W, ("image", "target_range"))
    pyr = Pyramid(H, W, 2, device)

    def call():
        images, ranges = pyr.build(image, rng_map)
        return {"image1": images[1], "image2": images[2], "range1": ranges[1], "range2": ranges[2]}

    run.call = call
    return run


def _range_maps(H, W, cam, seed):
    """A smooth range map of a curved surface in front of ``cam`` (positive, finite) and the alpha map of full cover."""
    rng = _rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    a, b, c = rng.uniform(0.1, 0.4, 3)
    rngm = 2.0 + a * np.sin(x / 9.0 + c) + b * np.cos(y / 7.0)
    return rngm.astype(np.float32), np.ones((H, W), np.float32)


def _icp(align):
    def build(device):
        from gs_icp import IcpAligner, IcpOptions

        run = Run(device)
        cam = _camera(W0, H0)
        (d0, a0), (d1, a1) = _range_maps(H0, W0, cam, 71), _range_maps(H0, W0, cam, 72)
        depth = run.input("depth", d0 * a0, d1 * a1)
        alpha = run.input("alpha", a0 * np.float32(0.999), a1)
        frame = run.input("range_map", d0 + np.float32(0.01), d1 - np.float32(0.02))
        icp = IcpAligner(cam, IcpOptions(stages=((2, 2), (1, 2))), device)

        def call():
            vertex, normal = icp.set_model(depth, alpha, cam.rot, cam.tran)
            out = {"vertex": vertex, "normal": normal}
            if align:
                icp.align(frame)
                out["state:state_and_log"] = icp._dev
            return out

        run.call = call
        return run

    return build


def _device_track(device):
    """gs_track.Tracker with the pose on the device: reset, then per iteration a device-pose forward, the tracking loss, the
    pose-only backward and gs_pose_step -- ``_enqueue_device_track`` ("nothing waits"), three iterations."""
    from gs_track import TrackOptions, Tracker

    run = Run(device)
    W, H, n = W0, H0, 5000
    params = _scene_inputs(run, n, W, H)
    image, _, _, _, rng_map = _maps(run, H, W, ("image", "target_range"))
    cam = _camera(W, H)
    tr = Tracker(params, cam, TrackOptions(iterations=3, device_pose=True, max_pairs=MAX_PAIRS), device)

    def call():
        stages, images, ranges, total = tr._stage_list(image, rng_map)
        nv = tr._values.numel()
        dp = tr._device_buffers(total, nv)
        tr._enqueue_device_track(cam.rot, cam.tran, stages, images, ranges, total, dp, nv)
        return {"state:pose_state_and_log": dp["dev"], "state:pose": dp["pose"], "state:grad_and_values": tr._dev}

    run.call = call
    run.check = _no_overflow(tr.renderer)
    return run


# ---------------------------------------------------------------------------------------------------- map editing
def _densify(device):
    import torch
    from gs_densify import densify_apply, densify_apply_state, densify_classify

    run = Run(device)
    n = 5000
    params = _scene_inputs(run, n, W0, H0)
    grad = _normal_input(run, "grad", (n, 3), (81, 82), 3e-4)
    moments = [_normal_input(run, f"moment{k}", (n, w), (83 + k, 93 + k)) for k, w in enumerate((3, 4))]
    draws = tuple(torch.from_numpy(_rng(s).standard_normal((n, 3)).astype(np.float32)).to(device) for s in (85, 86))
    cap = 3 * n
    out = [_zeros(device, cap, *t.shape[1:]) for t in params]
    dst = [_zeros(device, cap, *t.shape[1:]) for t in moments]

    def call():
        for t in (*out, *dst):
            t.zero_()
        counts, ws, opts = densify_classify(params, grad, 0.05, 0.17)
        densify_apply(params, grad, out, counts, ws, opts, draws, n, cap)
        densify_apply_state(moments, dst, n, counts, ws, cap)
        return {"counts": counts, **{f"out{k}": t for k, t in enumerate(out)}, **{f"state_out{k}": t for k, t in enumerate(dst)}}

    run.call = call
    return run


def _prune(contrib):
    def build(device):
        from gs_prune import contrib_options, prune_apply, prune_classify, prune_options

        run = Run(device)
        n = 5000
        params = _scene_inputs(run, n, W0, H0)
        rows = None
        if contrib:
            rows = run.input("contributions", *((np.abs(_rng(s).standard_normal((n, 4))) * [1, 1, 9, 2]).astype(np.float32)
                                                for s in (87, 88)))
        dst = [_zeros(device, n, *t.shape[1:]) for t in params]

        def call():
            for t in dst:
                t.zero_()
            opts = prune_options(opa_min=0.3, scale_max=None)
            if contrib:
                counts, ws = prune_classify(params[2], params[3], opts, rows, contrib_options(0.2, 2, 1))
            else:
                counts, ws = prune_classify(params[2], params[3], opts)
            prune_apply(params, dst, n, counts, ws)
            return {"counts": counts, **{f"dst{k}": t for k, t in enumerate(dst)}}

        run.call = call
        return run

    return build


def _seed(pp):
    def build(device):
        from gs_seed import seed_apply, seed_classify, seed_options

        run = Run(device)
        H, W = H0, W0
        image, depth, alpha, _, rng_map = _maps(run, H, W, ("image", "depth", "alpha", "target_range"))
        cam = _camera(W, H, pp=pp)
        cap = H * W
        out = [_zeros(device, cap, *s) for s in ((3,), (4,), (3,), (), (3,))]

        def call():
            for t in out:
                t.zero_()
            opts = seed_options(stride=2)
            counts, ws = seed_classify(rng_map, (depth, alpha), opts)
            seed_apply(image, rng_map, cam, opts, out, 0, counts, ws)
            return {"counts": counts, **{f"out{k}": t for k, t in enumerate(out)}}

        run.call = call
        return run

    return build


def _views(kind, pp):
    """gs_view_overlap / gs_view_redundancy of a range map against a table of four views (``pp``: an off-centre frame camera)."""
    def build(device):
        import torch
        from gs_slam import view_overlap, view_redundancy, view_row

        run = Run(device)
        H, W = H0, W0
        cam = _camera(W, H, pp=pp)
        rng_map = run.input("range_map", _range_maps(H, W, cam, 73)[0], _range_maps(H, W, cam, 74)[0] * np.float32(3.0))
        table = torch.from_numpy(np.stack([view_row(_camera(W, H, yaw=y)) for y in (2.0, 9.0, 25.0, -14.0)])).to(device)

        def call():
            if kind == "overlap":
                return {"counts": view_overlap(rng_map, cam, table, 4, stride=2)}
            return {"hist": view_redundancy(rng_map, cam, table, 4, self_index=0, stride=2)}

        run.call = call
        return run

    return build


# ---------------------------------------------------------------------------------------------------- the catalogue
_STATS_SYNC = 'FrameRenderer.stats: "Synchronises the current stream (one 32-byte D2H copy)."'
_ICP_SYNC = ('IcpAligner: "align(range_map, init) estimates the frame\'s pose: reset + two launches per iteration on the current '
             'stream, then ONE read of the state and the log."')

_PROFILE_SYNC = ('gs_abi.h, gs_frame_forward_profile: "brackets every stage with hipEvents on `stream` and returns the stage '
                 'durations in milliseconds (synchronises; for bench.py / profiling only)"; gs_frame_backward_profile: "Likewise"')

_FWD = ("gs_frame_forward",)
_FWD_BWD = ("gs_frame_forward", "gs_frame_backward")

CASES: List[Case] = [
    # reference API
    Case("ref_world2camera_jacobian", _ref_world2camera, ("gs_world2camera", "gs_jacobian", "gs_world2camera_backward")),
    Case("ref_global_culling", _ref_global_culling, ("gs_global_culling", "gs_global_culling_backward")),
    *[Case(f"ref_calc_tile_list_method{m}", _ref_calc_tile_list(m), ("gs_calc_tile_list",)) for m in (2, 1, 0)],
    Case("ref_gather", _ref_gather, ("gs_gather_gaussians",)),
    Case("ref_draw_rgb", _ref_draw(False, False, True), ("gs_draw", "gs_draw_backward")),
    Case("ref_draw_sh", _ref_draw(True, False, True), ("gs_draw", "gs_draw_backward")),
    Case("ref_draw_rgb_sigmoid", _ref_draw(False, True, True), ("gs_draw", "gs_draw_backward")),
    Case("ref_draw_rgb_exact_exp", _ref_draw(False, False, False), ("gs_draw", "gs_draw_backward")),
    *[Case(f"sort_pairs_n{n}", _sort(n, False), ("gs_sort_pairs",)) for n in (2049, SORT_ONE_TRIP + 1)],
    *[Case(f"sort_pairs_bits_n{n}", _sort(n, True), ("gs_sort_pairs_bits",)) for n in (2049, SORT_ONE_TRIP + 1)],
    # frame path: inference
    *[Case(f"frame_rgb_strips{int(fs)}_sort{sm}", _frame_inference(W0, H0, 5000, force_strips=fs, sort_mode=sm), _FWD)
      for fs, sm in ((True, 2), (False, 2), (True, 1), (True, 0))],
    Case("frame_rgb_larger", _frame_inference(W1, H1, 6000), _FWD),
    Case("frame_sh2", _frame_inference(W0, H0, 4000, sh=2), _FWD),
    Case("frame_sh3_table", _frame_inference(W1, H1, 4000, sh=3, force_strips=False), _FWD),
    Case("frame_aux", _frame_inference(W0, H0, 5000, aux=True), _FWD),
    Case("frame_principal_point", _frame_inference(W0, H0, 5000, pp=True), _FWD),
    Case("frame_scene_pack", _frame_inference(W0, H0, 5000, frames=3, scene_pack=None), ("gs_frame_forward", "gs_scene_pack_build")),
    Case("frame_occlusion_culled", _frame_inference(W0, H0, 5000, frames=4, occlusion_cull=True, cull_second_pass="always"),
         ("gs_frame_forward", "gs_frame_stats_tagged_async")),
    Case("frame_cull_repeat", _frame_cull_repeat, ("gs_frame_forward", "gs_scene_pack_build", "gs_frame_stats_tagged_async")),
    Case("frame_counters", _frame_counters, ("gs_frame_stats_async", "gs_frame_longest_list_async",
                                             "gs_frame_cull_fallback_async", "gs_frame_stats_tagged_async")),
    Case("frame_stats", _frame_stats, ("gs_frame_stats_tagged_async",), synchronising=_STATS_SYNC),
    Case("frame_profile", _frame_profile, ("gs_frame_forward_profile", "gs_frame_backward_profile"), synchronising=_PROFILE_SYNC),
    # frame path: training
    Case("train_pixel", _frame_training(W0, H0, 5000, bwd_rows=False), _FWD_BWD),
    Case("train_pixel_larger_table", _frame_training(W1, H1, 6000, bwd_rows=False, force_strips=False), _FWD_BWD),
    Case("train_rows", _frame_training(W0, H0, 5000, bwd_rows=True), _FWD_BWD),
    Case("train_sh2_matrix_pipe", _frame_training(W0, H0, 4000, sh=2), _FWD_BWD),
    Case("train_sh3_matrix_pipe", _frame_training(W0, H0, 4000, sh=3), _FWD_BWD),
    Case("train_aux", _frame_training(W0, H0, 5000, aux=True), _FWD_BWD),
    Case("train_principal_point", _frame_training(W0, H0, 5000, pp=True, bwd_rows=False), _FWD_BWD),
    Case("train_backward_parts", _frame_training(W0, H0, 5000, mode="parts", bwd_rows=False),
         ("gs_frame_forward", "gs_frame_backward_part")),
    Case("train_backward_slices", _frame_training(W0, H0, 5000, mode="slices", bwd_rows=False),
         ("gs_frame_backward_part", "gs_frame_backward_slice")),
    Case("train_forward_in_slices", _frame_training(W0, H0, 5000, mode="begin", bwd_rows=False, auto_grow="async"),
         ("gs_frame_forward_project", "gs_frame_forward_rest", "gs_frame_backward")),
    Case("train_fused_adam", _frame_fused_adam(W0, H0, 5000, "plain"), ("gs_frame_forward", "gs_frame_backward_adam")),
    Case("train_fused_adam_aux", _frame_fused_adam(W0, H0, 5000, "aux"), ("gs_frame_forward", "gs_frame_backward_adam_aux")),
    Case("train_fused_adam_pose", _frame_fused_adam(W0, H0, 5000, "pose"), ("gs_frame_forward", "gs_frame_backward_adam_pose")),
    Case("train_pose_only", _frame_pose_only, ("gs_frame_forward", "gs_frame_backward_pose")),
    Case("train_device_pose", _frame_device_pose, ("gs_frame_forward", "gs_frame_backward_pose")),
    Case("train_contrib", _frame_contrib, ("gs_frame_forward", "gs_frame_contrib")),
    # the library's own side stream
    Case("side_stream_same", _side_stream("same"), ("gs_frame_forward", "gs_loss_l1_ssim", "gs_frame_backward")),
    Case("side_stream_backward_on_second", _side_stream("backward"), ("gs_frame_forward", "gs_loss_l1_ssim", "gs_frame_backward")),
    Case("side_stream_release_and_grow", _side_stream("release"), ("gs_frame_forward", "gs_frame_async_wait", "gs_frame_backward")),
    # training-step kernels
    Case("image_loss_31x33", _image_loss(31, 33), ("gs_loss_l1_ssim",)),
    Case("image_loss_53x483", _image_loss(53, 483), ("gs_loss_l1_ssim",)),
    Case("weighted_image_loss", _image_loss(53, 483, weighted=True), ("gs_loss_l1_ssim_weighted",)),
    Case("depth_loss", _depth_loss, ("gs_loss_depth",)),
    Case("track_loss", _track_loss("plain"), ("gs_loss_track",)),
    Case("track_loss_gated", _track_loss("gated"), ("gs_loss_track_gated",)),
    Case("gate_mask", _track_loss("mask"), ("gs_track_gate_mask",)),
    Case("adam_step", _adam("one"), ("gs_adam_step",)),
    Case("adam_step_range", _adam("range"), ("gs_adam_step_range",)),
    *[Case(f"adam_step_sharded_skip{k}", _adam("sharded", k), ("gs_adam_step_sharded",)) for k in (0, 1)],
    *[Case(f"adam_step_multi_skip{k}", _adam("multi", k), ("gs_adam_step_multi",)) for k in (0, 1)],
    Case("grad_stat_update", _grad_stat, ("gs_grad_stat_update",)),
    Case("exposure_fixed", _exposure(False), ("gs_exposure_apply", "gs_exposure_backward")),
    Case("exposure_free", _exposure(True), ("gs_exposure_apply", "gs_exposure_backward")),
    Case("pyramid_down", _pyramid, ("gs_pyramid_down",)),
    Case("icp_model_maps", _icp(False), ("gs_icp_model_maps",)),
    Case("icp_align", _icp(True), ("gs_icp_model_maps", "gs_icp_reset", "gs_icp_step"), synchronising=_ICP_SYNC),
    Case("device_pose_track", _device_track, ("gs_pose_reset", "gs_pose_step", "gs_frame_forward", "gs_loss_track",
                                              "gs_frame_backward_pose")),
    # map editing
    Case("densify", _densify, ("gs_densify_classify", "gs_densify_apply", "gs_densify_apply_state")),
    Case("prune", _prune(False), ("gs_prune_classify", "gs_prune_apply")),
    Case("prune_contrib", _prune(True), ("gs_prune_classify_contrib", "gs_prune_apply")),
    Case("seed", _seed(False), ("gs_seed_classify", "gs_seed_apply")),
    Case("seed_principal_point", _seed(True), ("gs_seed_classify", "gs_seed_apply_pp")),
    Case("view_overlap", _views("overlap", False), ("gs_view_overlap",)),
    Case("view_overlap_principal_point", _views("overlap", True), ("gs_view_overlap_pp",)),
    Case("view_redundancy", _views("redundancy", False), ("gs_view_redundancy",)),
    Case("view_redundancy_principal_point", _views("redundancy", True), ("gs_view_redundancy_pp",)),
]

# Entry points without a case, each with its reason (at most EXEMPT_MAX; never a forward, a backward, a loss, Adam or exposure).
EXEMPT_MAX = 6
EXEMPT: Dict[str, str] = {}  # (none today: the two _profile entry points have a synchronising case of their own)
