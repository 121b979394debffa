"""The Python layer's shared plumbing, without a device: gs_call (device refusal, tensor check), gaussian._lib.call, and the
poses and posed cameras of gs_geometry.  No kernel is launched."""
import ast

import numpy as np
import pytest
import torch

import gs_call
import gs_geometry
from gaussian import _lib


def test_gs_call_imports_torch_alone():
    """Importable without a device and without gs_frame: its only import is torch."""
    tree = ast.parse(open(gs_call.__file__).read())
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names == {"torch", "__future__"}


def test_require_hip():
    with pytest.raises(RuntimeError) as e:
        gs_call.require_hip("cpu", "X")
    assert str(e.value) == "X needs a HIP device; there is no CPU fallback"
    with pytest.raises(RuntimeError, match="^the overlap count needs a HIP device; there is no CPU fallback$"):
        gs_call.require_hip(torch.device("cpu"), "the overlap count")
    dev = gs_call.require_hip("cuda:1", "X")  # (naming a device initialises nothing)
    assert isinstance(dev, torch.device) and (dev.type, dev.index) == ("cuda", 1)


def test_check_tensor_names_the_argument_and_prints_one_shape_format():
    t = torch.zeros(8, 8)  # float32 and contiguous, but on the CPU
    base = "must be a contiguous float32 HIP tensor"
    for kwargs, tail in ((dict(shape=(8, 8)), " of shape [8, 8]"), (dict(shape=(44, 60, 3)), " of shape [44, 60, 3]"),
                         (dict(rows_min=5, tail=(16,)), " of shape [>= 5, 16]"), (dict(rows_min=5, tail=()), " of shape [>= 5]"),
                         (dict(rows_min=5), " of shape [>= 5, ...]"), ({}, "")):
        with pytest.raises(RuntimeError) as e:
            gs_call.check_tensor("table", t, **kwargs)
        assert str(e.value) == f"table {base}{tail}"
    with pytest.raises(RuntimeError) as e:
        gs_call.check_tensor("grad_rot", t, (3, 3), device=torch.device("cuda", 0))
    assert str(e.value) == f"grad_rot {base} of shape [3, 3] on the same device as cuda:0"


def test_lib_call_resolves_the_symbol_when_called_and_names_it(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "gs_prune_classify", lambda *a: seen.append(a) or 7)
    monkeypatch.setattr(_lib, "gs_last_error", lambda: b"the fake said no")
    with pytest.raises(RuntimeError) as e:
        _lib.call("gs_prune_classify", 1, None, "x")
    assert seen == [(1, None, "x")]
    assert str(e.value) == "gs_prune_classify failed (code 7): the fake said no"
    monkeypatch.setattr(_lib, "gs_prune_classify", lambda *a: 0)
    assert _lib.call("gs_prune_classify") is None
    with pytest.raises(KeyError):
        _lib.call("gs_no_such_symbol")


def test_stream_looks_the_current_stream_up_when_called(monkeypatch):
    class Stream:
        cuda_stream = 1234

    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: Stream())
    assert gs_call.stream() == 1234


def _pose(seed=0):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q, rng.standard_normal(3)


def test_pose64_takes_lists_arrays_and_tensors_and_returns_fresh_float64():
    rot, tran = _pose()
    rot32, tran32 = rot.astype(np.float32), tran.astype(np.float32)
    for r, t in ((rot32.tolist(), tran32.tolist()), (rot32, tran32), (torch.from_numpy(rot32), torch.from_numpy(tran32)),
                 (rot32.reshape(9), tran32.reshape(3, 1)), (rot, tran)):
        R, T = gs_geometry.pose64(r, t)
        assert R.dtype == T.dtype == np.float64 and R.shape == (3, 3) and T.shape == (3,)
        want = rot if r is rot else rot32
        assert np.array_equal(R, np.asarray(want, np.float64).reshape(3, 3))
        for out, src in ((R, r), (T, t)):
            if not isinstance(src, list):
                assert not np.shares_memory(out, src.numpy() if torch.is_tensor(src) else src)
    R, _ = gs_geometry.pose64(rot, tran)
    R[0, 0] = 5.0
    assert rot[0, 0] != 5.0


class _Cam:
    def __init__(self, rot, tran):
        self.width, self.height, self.focal_x, self.focal_y, self.near = 8, 8, 10.0, 10.0, 0.3
        self.rot, self.tran = rot, tran


def test_posed_never_aliases_and_rounds_like_ascontiguousarray():
    rot0, tran0 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    cam = _Cam(rot0, tran0)
    rot, tran = _pose(1)
    for r, t in ((rot, tran), (rot.astype(np.float32), tran.astype(np.float32)),  # the second: what ascontiguousarray aliased
                 (np.asfortranarray(rot), tran), (rot.tolist(), tran.tolist())):
        c = gs_geometry.posed(cam, r, t)
        assert c is not cam and cam.rot is rot0 and cam.tran is tran0 and (c.width, c.near) == (8, 0.3)
        assert c.rot.dtype == c.tran.dtype == np.float32 and c.rot.shape == (3, 3) and c.tran.shape == (3,)
        assert c.rot.flags["C_CONTIGUOUS"] and c.tran.flags["C_CONTIGUOUS"]
        assert c.rot.tobytes() == np.ascontiguousarray(r, np.float32).tobytes()
        assert c.tran.tobytes() == np.ascontiguousarray(t, np.float32).tobytes()
        if isinstance(r, np.ndarray):
            assert not np.shares_memory(c.rot, r) and not np.shares_memory(c.tran, t)
    assert np.array_equal(rot0, np.eye(3))


def test_pose_ctypes_is_the_float32_pose_row_major():
    rot, tran = _pose(2)
    r9, t3 = gs_geometry.pose_ctypes(_Cam(rot, tran))
    assert len(r9) == 9 and len(t3) == 3
    assert bytes(r9) == np.ascontiguousarray(rot, np.float32).tobytes()
    assert bytes(t3) == np.ascontiguousarray(tran, np.float32).tobytes()
