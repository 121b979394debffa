"""CPU tier of the fused training step with a pose gradient (include/gs_abi.h: gs_frame_backward_adam_pose): the symbol and
its binding, every refusal on fake pointers (each comes before anything is enqueued), the unchanged refusals of the two older
fused entry points, the pose optimizer extracted from Tracker.track (gs_track.PoseAdam) bit for bit against a restatement of
the loop body it came from, lazy against eager application of pose updates (gs_track.FreePose), and the registers / scratch
of the four new kernel instantiations read from the built code objects.  No kernel is launched."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from gs_testutil import FAKE, fake_adam as _adam
from test_pose_host import GS_E_INVALID, GS_E_UNSUPPORTED, _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIMG = FAKE + (9 << 30)


# ------------------------------------------------------------------------------------------------------------ 1. the C ABI
def test_symbol_is_exported_and_bound():
    from gaussian import _lib

    assert "gs_frame_backward_adam_pose" in _lib.EXPORTS
    assert getattr(_lib.lib, "gs_frame_backward_adam_pose") is not None
    assert callable(_lib.gs_frame_backward_adam_pose)
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    assert "int gs_frame_backward_adam_pose(" in header
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays


@pytest.mark.parametrize("aux", [False, True])
def test_refusals_come_before_any_launch(aux):
    from gaussian import _lib

    call = _lib.gs_frame_backward_adam_pose
    # SH colours: the sentence of the plain backward
    for cd in (27, 48):
        assert call(C.byref(_frame(aux=aux, color_dim=cd)), GIMG, C.byref(_adam()), None) == GS_E_UNSUPPORTED
        msg = _lib.gs_last_error()
        assert b"GS_FRAME_POSE_GRAD needs rgb colours" in msg and b"ray directions" in msg
    # a frame without the flag: the older entry points are its
    assert call(C.byref(_frame(pose=False, aux=aux)), GIMG, C.byref(_adam()), None) == GS_E_INVALID
    assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()
    # the pose fields go through the frame's validation
    f = _frame(aux=aux)
    f.pose_workspace = None
    assert call(C.byref(f), GIMG, C.byref(_adam()), None) == GS_E_INVALID
    f = _frame(aux=aux)
    f.grad_tran = None
    assert call(C.byref(f), GIMG, C.byref(_adam()), None) == GS_E_INVALID
    # not a training frame
    assert call(C.byref(_frame(aux=aux, training=0)), GIMG, C.byref(_adam()), None) == GS_E_INVALID
    assert b"training" in _lib.gs_last_error()
    # no optimizer descriptor; step 0 (the all-zero descriptor); a bad beta; a missing and a misaligned moment
    assert call(C.byref(_frame(aux=aux)), GIMG, None, None) == GS_E_INVALID
    assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(_adam(good=False)), None) == GS_E_INVALID
    a = _adam()
    a.step = 0
    assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(a), None) == GS_E_INVALID
    assert b"step" in _lib.gs_last_error()
    a = _adam()
    a.beta2 = 1.0
    assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(a), None) == GS_E_INVALID
    a = _adam()
    a.exp_avg_sq[3] = None
    assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(a), None) == GS_E_INVALID
    for k in (0, 1, 2, 4):
        a = _adam()
        a.exp_avg[k] = a.exp_avg[k] + 4
        assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(a), None) == GS_E_INVALID
        assert b"16-byte aligned" in _lib.gs_last_error()
    a = _adam()
    a.stat_mode = 1  # a statistic without its array
    assert call(C.byref(_frame(aux=aux)), GIMG, C.byref(a), None) == GS_E_INVALID
    # a NULL image is the zero image of aux frames only
    if not aux:
        assert call(C.byref(_frame()), None, C.byref(_adam()), None) == GS_E_INVALID


def test_the_older_fused_entry_points_still_refuse_flagged_frames():
    from gaussian import _lib

    assert _lib.gs_frame_backward_adam(C.byref(_frame()), GIMG, C.byref(_adam()), None) == GS_E_UNSUPPORTED
    assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()
    assert _lib.gs_frame_backward_adam_aux(C.byref(_frame(aux=True)), GIMG, C.byref(_adam()), None) == GS_E_UNSUPPORTED
    assert b"GS_FRAME_POSE_GRAD" in _lib.gs_last_error()


# ---------------------------------------------------------------------------------------------------- 2. the pose optimizer
def _gradients(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=9) * 10.0 ** rng.uniform(-3, 1), rng.normal(size=3) * 10.0 ** rng.uniform(-3, 1))
            for _ in range(n)]


def _start(seed):
    from gs_track import so3_exp

    rng = np.random.default_rng(seed)
    return so3_exp(rng.normal(size=3) * 0.4), rng.normal(size=3)


def _parent_loop(R, t, grads, lr_rot, lr_tran, lr_final, betas, eps, iterations):
    """The loop body of Tracker.track as it stood before the step became gs_track.PoseAdam, written out: the gradient of
    iteration k is grads[k] instead of a rendered frame's."""
    from gs_track import rot_tangent_grad, so3_exp

    m, v = np.zeros(6), np.zeros(6)
    lr0 = np.array([lr_rot] * 3 + [lr_tran] * 3)
    b1, b2 = betas
    out = []
    for k in range(len(grads)):
        h = np.concatenate([grads[k][0], grads[k][1]]).astype(np.float64)
        g = np.concatenate([rot_tangent_grad(h[0:9], R), h[9:12]])
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        step = lr0 * lr_final ** (k / iterations) * (m / (1.0 - b1 ** (k + 1))) / (np.sqrt(v / (1.0 - b2 ** (k + 1))) + eps)
        R = so3_exp(-step[:3]) @ R
        t = t - step[3:]
        out.append((R, t))
    return out


def test_pose_adam_is_the_trackers_step_bit_for_bit():
    from gs_track import PoseAdam, TrackOptions

    o = TrackOptions()
    grads = _gradients(20, 5)
    R0, t0 = _start(6)
    want = _parent_loop(R0, t0, grads, o.lr_rot, 3e-3, o.lr_final, o.betas, o.eps, o.iterations)
    adam = PoseAdam(R0, t0, o.lr_rot, 3e-3, o.betas, o.eps)
    for k, (gr, gt) in enumerate(grads):
        h = np.concatenate([gr, gt]).astype(np.float64)
        R, t = adam.step(h[0:9], h[9:12], o.lr_final ** (k / o.iterations))
        assert np.array_equal(R, want[k][0]) and np.array_equal(t, want[k][1]), k
        assert adam.k == k + 1
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
    assert not np.array_equal(want[-1][0], R0) and not np.array_equal(want[-1][1], t0)
    # the Trainer's use (no decay): a scale of one is the plain rate
    a1, a2 = PoseAdam(R0, t0, 1e-3, 2e-3), PoseAdam(R0, t0, 1e-3, 2e-3)
    for gr, gt in grads:
        a1.step(gr, gt)
        a2.step(gr, gt, 1.0)
    assert np.array_equal(a1.rot, a2.rot) and np.array_equal(a1.tran, a2.tran)
    # rates of zero leave the pose bit-unchanged, whatever the gradient
    z = PoseAdam(R0, t0, 0.0, 0.0)
    for gr, gt in grads:
        z.step(gr, gt)
    assert np.array_equal(z.rot, R0) and np.array_equal(z.tran, t0)


def test_lazy_application_equals_eager_application():
    """Three interleaved views whose gradient depends on the pose it is taken at (as a rendered frame's does): applying every
    update at once, and applying it only when the view's pose is read next, end in identical float64 poses."""
    from gs_track import FreePose, PoseAdam

    order = [0, 1, 2, 1, 0, 2, 2, 0, 1, 0, 1, 2, 0, 0, 1, 2, 2, 1]
    A = np.random.default_rng(8).normal(size=(3, 12, 12))

    def gradient(view, rot, tran):  # any deterministic function of the pose
        x = np.concatenate([rot.reshape(9), tran])
        return np.tanh(A[view] @ x).astype(np.float32)

    def run(lazy):
        views = [FreePose(PoseAdam(*_start(20 + i), 2e-3, 1e-3)) for i in range(3)]
        reads = []
        for v in order:
            fp = views[v]
            fp.settle()  # the reader: the pose of the previous step on this view
            reads.append((fp.adam.rot.copy(), fp.adam.tran.copy()))
            fp.host.copy_(torch.from_numpy(gradient(v, fp.adam.rot, fp.adam.tran)))
            fp.deliver()
            if not lazy:
                assert fp.settle() and not fp.pending
            else:
                assert fp.pending
        for fp in views:
            fp.settle()
        return views, reads

    (eager, reads_e), (lazy, reads_l) = run(False), run(True)
    for a, b in zip(eager, lazy):
        assert np.array_equal(a.adam.rot, b.adam.rot) and np.array_equal(a.adam.tran, b.adam.tran)
        assert a.adam.k == b.adam.k == 6 and not a.settle() and not b.settle()
    for (ra, ta), (rb, tb) in zip(reads_e, reads_l):
        assert np.array_equal(ra, rb) and np.array_equal(ta, tb)
    assert not np.array_equal(eager[0].adam.rot, _start(20)[0])


# ------------------------------------------------------------------------------------- 3. the kernels' registers and scratch
# From the code objects of the first build: the plain variant 77 VGPRs -- the aux-Adam kernel's own
# count, six waves per SIMD --, the aux variant 93 (the register file holds five waves of it).  No scratch, no spills.
POSE_ADAM_VGPRS = [("ILb0ELi1E", 77), ("ILb0ELi2E", 77), ("ILb1ELi1E", 93), ("ILb1ELi2E", 93)]


@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def test_there_are_exactly_four_instantiations(kernels):
    names = [k for k in kernels if "frame_project_backward_adam_pose_kernel" in k]
    assert len(names) == 4, names
    assert sorted(t for t, _ in POSE_ADAM_VGPRS) == sorted(n.split("frame_project_backward_adam_pose_kernel")[1][:9]
                                                           for n in names)


@pytest.mark.parametrize("inst,vgprs", POSE_ADAM_VGPRS, ids=[t for t, _ in POSE_ADAM_VGPRS])
def test_pose_adam_kernel_resources(kernels, inst, vgprs):
    hits = [k for k in kernels if "frame_project_backward_adam_pose_kernel" + inst in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0, k[".name"]
    assert k[".vgpr_count"] == vgprs, (k[".name"], k[".vgpr_count"])
    assert k[".max_flat_workgroup_size"] == 256
    # two 192-byte pose rows on top of the aux-Adam kernel's LDS: still seven workgroups of 256 per CU
    aux = [n for n in kernels if "frame_project_backward_adam_aux_kernelILi3ELi256ELi1E" in n]
    assert len(aux) == 1
    lds = k[".group_segment_fixed_size"]
    assert lds <= kernels[aux[0]][".group_segment_fixed_size"] + 384 and lds * 7 <= 160 * 1024
    assert min(8, 512 // (math.ceil(vgprs / 8) * 8)) == (6 if vgprs == 77 else 5)
