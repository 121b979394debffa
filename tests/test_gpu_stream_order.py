"""GPU tier of the stream-order tests: every case of tests/stream_order.py on a stream whose inputs arrive late, bit for bit
against its default-stream run (the kernels are bitwise repeatable by design), with the Python layer's stream argument
recorded on the way.  The harness, its two safeguards and the catalogue are described in tests/stream_order.py.

GS_STREAM_ORDER_REPORT=<path>: write the calibration, the per-case host times and delays and the synchronising cases there
(profiles/stream_order.txt was recorded that way)."""
import os

import pytest
import torch

import stream_order as so

pytestmark = pytest.mark.gpu

ENTRY_POINTS = so.stream_entry_points()


@pytest.fixture(scope="module")
def session(gpu):
    """The delay, calibrated once, and the positive control: without it the module fails, it does not skip."""
    s = so.calibrate(gpu)
    so.choose_streams(s, gpu)
    so.positive_control(s, gpu)
    yield s
    path = os.environ.get("GS_STREAM_ORDER_REPORT")
    if path:
        so.write_report(s, so.CASES + [TWO_RENDERERS], path)


def record_streams(monkeypatch, allowed, seen):
    """Every stream-taking ``gaussian._lib.gs_*`` behind a wrapper: while a delayed run is being issued (``allowed`` holds its
    stream handles) the last argument must be the current stream's handle, and that one of them; then it calls through."""
    from gaussian import _lib

    for name in ENTRY_POINTS:
        def wrapper(*args, _fn=getattr(_lib, name), _name=name):
            if allowed:
                cur = torch.cuda.current_stream().cuda_stream
                assert args[-1] == cur and cur in allowed, (
                    f"{_name} was handed stream {args[-1]!r}; the current stream is {cur!r}, the case's streams {sorted(allowed)}")
                seen.add(_name)
            return _fn(*args)

        monkeypatch.setattr(_lib, name, wrapper)


@pytest.mark.parametrize("case", so.CASES, ids=[c.name for c in so.CASES])
def test_stream_order(gpu, session, monkeypatch, case):
    allowed, seen = set(), set()
    record_streams(monkeypatch, allowed, seen)
    try:
        so.run_case(case, gpu, session, allowed)
    except RuntimeError as e:  # a device that faulted answers nothing any more: the cases behind this one are not started on it
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"{case.name}: the device reported {e}", returncode=3)
        raise
    assert set(case.covers) <= seen, f"{case.name} claims {sorted(set(case.covers) - seen)} and never called them"


TWO_RENDERERS = so.Case("two_renderers_at_once", None, ("gs_frame_forward", "gs_frame_backward", "gs_frame_backward_adam_aux"))


def test_two_renderers_interleave_behind_one_delay(gpu, session, monkeypatch):
    """Two FrameRenderers with different scenes, each a training forward + backward on a stream of its own, both streams held
    by the SAME delay so that their kernels really interleave; each against its own default-stream run.  What it is after is
    state the library shares between callers: one renderer takes gs_frame_backward_adam_aux with ``grad_image=None``, which
    reads the one-per-device zero image, while the other's backward is in flight."""
    import time

    cases = [so.Case("two_renderers_at_once/fused_adam_aux", so._frame_fused_adam(so.W0, so.H0, 5000, "aux", seeds=(13, 14)),
                     ("gs_frame_forward", "gs_frame_backward_adam_aux")),
             so.Case("two_renderers_at_once/train_aux", so._frame_training(so.W0, so.H0, 4000, aux=True, seeds=(15, 16)),
                     ("gs_frame_forward", "gs_frame_backward"))]
    allowed, seen = set(), set()
    record_streams(monkeypatch, allowed, seen)
    t_wall = time.perf_counter()
    with torch.cuda.device(gpu):
        base = [so.baseline(c, gpu) for c in cases]
        delay_ms = max(so.delay_for(c, host_ms, session) for c, (_, host_ms) in zip(cases, base))
        streams = [session.S, session.S2]  # (screened: neither shares a hardware queue with the other or the default stream)
        runs = []
        for c, S in zip(cases, streams):
            with torch.cuda.stream(S):
                allowed.add(S.cuda_stream)
                runs.append(c.build(gpu))
                so._warm_up(runs[-1])
                allowed.clear()
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            session.delay(delay_ms)
            released = torch.cuda.Event()
            released.record()
        streams[1].wait_event(released)
        late = []
        for run, S in zip(runs, streams):
            with torch.cuda.stream(S):
                allowed.add(S.cuda_stream)
                late.append(so.late_call(run, S))
                allowed.clear()
        torch.cuda.synchronize()
        for c, run, (snap, held), (want, _) in zip(cases, runs, late, base):
            so.compare(c, run, snap, want, held, delay_ms)
    assert set(TWO_RENDERERS.covers) <= seen
    session.delay_ms[TWO_RENDERERS.name] = delay_ms
    session.wall_s[TWO_RENDERERS.name] = time.perf_counter() - t_wall
