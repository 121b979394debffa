"""CPU tier of the device-resident pose (GS_FRAME_DEVICE_POSE with gs_frame_dp, gs_pose_step / gs_pose_reset / gs_pose_log_bytes;
include/gs_abi.h): every refusal through the library on fake pointers -- so nothing here can have been enqueued --, the
layout of gs_frame_dp / gs_pose_state / gs_pose_step_opts between header and ctypes, the Python restatement of the step
(tests/pose_step_ref.py) against gs_track.PoseAdam, the Tracker's option, and the resources of the new kernels read from the
built code object against their by-value twins."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_step_ref
from gs_testutil import FAKE, fake_adam, fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2
POSE = FAKE + (10 << 30)


def _err():
    from gaussian import _lib

    return _lib.gs_last_error().decode()


def _frame(pose_dev=POSE, flagged=True, **kw):
    """fake_frame as a gs_frame_dp, flagged GS_FRAME_DEVICE_POSE."""
    from gaussian import _lib

    kw.setdefault("pose", True)
    src = fake_frame(**kw)
    f = _lib.GsFrameDP()
    C.memmove(C.byref(f), C.byref(src), C.sizeof(_lib.GsFrame))
    f.pose_dev = pose_dev
    if flagged:
        f.flags |= _lib.GS_FRAME_DEVICE_POSE
    return f


def _grads():
    return [FAKE + (8 << 30) + k * (1 << 24) for k in range(5)]


# ------------------------------------------------------------------------------------------------------ the flag and the struct
def test_flag_is_the_next_free_bit_and_the_abi_is_additive():
    from gaussian import _lib

    assert _lib.GS_FRAME_DEVICE_POSE == 32768 == 2 * _lib.GS_FRAME_PRINCIPAL_POINT
    assert _lib.gs_abi_version() == 8
    for name in ("gs_pose_log_bytes", "gs_pose_reset", "gs_pose_step"):
        assert name in _lib.EXPORTS and getattr(_lib.lib, name) is not None


_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gs_abi.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\n", sizeof(gs_frame), sizeof(gs_frame_scene), sizeof(gs_frame_pp), sizeof(gs_frame_dp),
           offsetof(gs_frame_dp, pose_dev));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gs_pose_state), offsetof(gs_pose_state, R),
           offsetof(gs_pose_state, t), offsetof(gs_pose_state, m), offsetof(gs_pose_state, v), offsetof(gs_pose_state, best_R),
           offsetof(gs_pose_state, best_t), offsetof(gs_pose_state, best_loss), offsetof(gs_pose_state, steps),
           offsetof(gs_pose_state, best_row), offsetof(gs_pose_state, skipped), offsetof(gs_pose_state, bad));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(gs_pose_step_opts), offsetof(gs_pose_step_opts, lr_rot),
           offsetof(gs_pose_step_opts, lr_tran), offsetof(gs_pose_step_opts, lr_scale), offsetof(gs_pose_step_opts, beta1),
           offsetof(gs_pose_step_opts, beta2), offsetof(gs_pose_step_opts, eps), offsetof(gs_pose_step_opts, track_best),
           offsetof(gs_pose_step_opts, n_values));
    printf("%d %d\n", GS_FRAME_DEVICE_POSE, GS_POSE_LOG_HEAD);
    return 0;
}
"""


def test_ctypes_mirrors_match_the_header(tmp_path):
    from gaussian import _lib

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on PATH")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(_LAYOUT_C)
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    frame, state, opts, consts = ([int(x) for x in line.split()] for line in
                                  subprocess.check_output([str(exe)]).decode().splitlines())
    assert frame == [C.sizeof(_lib.GsFrame), C.sizeof(_lib.GsFrameScene), C.sizeof(_lib.GsFramePP), C.sizeof(_lib.GsFrameDP),
                     _lib.GsFrameDP.pose_dev.offset]
    assert frame[4] == frame[2]  # the new field sits right behind gs_frame_pp, whose size did not change
    S = _lib.GsPoseState
    assert state == [C.sizeof(S)] + [getattr(S, n).offset for n in ("R", "t", "m", "v", "best_R", "best_t", "best_loss", "steps",
                                                                    "best_row", "skipped", "bad")]
    assert state[0] == 37 * 8 + 16
    O = _lib.GsPoseStepOpts
    assert opts == [C.sizeof(O)] + [getattr(O, n).offset for n in ("lr_rot", "lr_tran", "lr_scale", "beta1", "beta2", "eps",
                                                                   "track_best", "n_values")]
    assert consts == [_lib.GS_FRAME_DEVICE_POSE, _lib.GS_POSE_LOG_HEAD]


# ------------------------------------------------------------------------------------------------------ refusals of a flagged frame
def test_a_well_formed_flagged_frame_validates_on_the_host():
    from gaussian import _lib

    for kw in ({}, {"aux": True}, {"pose": False}, {"N": 0}):
        assert _lib.gs_frame_binning_variant(C.byref(_frame(**kw))) >= 0, _err()
    # without the flag the field is not read
    assert _lib.gs_frame_binning_variant(C.byref(_frame(pose_dev=None, flagged=False))) >= 0


def test_null_or_misaligned_pose_is_invalid_ahead_of_everything_else():
    from gaussian import _lib

    for bad in (None, POSE + 4, POSE + 8):
        # ... also where the frame is one a flagged frame cannot be: the pointer's rule is the first that applies
        for kw in ({}, {"training": 0}, {"color_dim": 27}):
            f = _frame(pose_dev=bad, **kw)
            assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
            assert "GS_FRAME_DEVICE_POSE: pose_dev null or not 16-byte aligned" in _err()
            assert _lib.gs_frame_forward(C.byref(f), None) == GS_E_INVALID
            assert _lib.gs_frame_backward_pose(C.byref(f), FAKE, 0, None) == GS_E_INVALID


def _unsupported_frames():
    from gaussian import _lib

    out = {"inference": _frame(training=0, pose=False), "sh2": _frame(color_dim=27, pose=False),
           "sh3": _frame(color_dim=48, pose=False)}
    for mode in (0, 1):
        f = _frame()
        f.sort_mode = mode
        out[f"sort_mode{mode}"] = f
    for name, flag in (("cull", _lib.GS_FRAME_OCCLUSION_CULL), ("slice_sort", _lib.GS_FRAME_SLICE_SORT)):
        f = _frame()
        f.flags |= flag
        out[name] = f
    f = _frame()  # (a scene pack on a training frame: GS_E_INVALID without the new flag -- the new flag's rule comes first)
    f.flags |= _lib.GS_FRAME_SCENE_PACK
    f.scene_pack_a, f.scene_pack_b, f.scene_pack_a_bytes, f.scene_pack_b_bytes = FAKE + (11 << 30), FAKE + (12 << 30), 1 << 20, 1 << 22
    out["scene_pack"] = f
    return out


def test_frames_a_flagged_frame_cannot_be_are_unsupported():
    from gaussian import _lib

    for name, f in _unsupported_frames().items():
        for rc in (_lib.gs_frame_forward(C.byref(f), None), _lib.gs_frame_backward_pose(C.byref(f), FAKE, 0, None),
                   _lib.gs_frame_binning_variant(C.byref(f))):
            assert rc == GS_E_UNSUPPORTED, (name, rc, _err())
            assert "GS_FRAME_DEVICE_POSE" in _err()
    # each is the frame it was without the flag
    f = _frame(training=0, pose=False, flagged=False)
    assert _lib.gs_frame_binning_variant(C.byref(f)) >= 0


def test_every_other_entry_point_refuses_a_flagged_frame():
    from gaussian import _lib

    f, P = _frame(), C.byref
    adam = fake_adam()
    ms6, ms3 = (C.c_float * 6)(), (C.c_float * 3)()
    ptrs = [C.c_void_p() for _ in range(7)]
    opts = _lib.GsContribOpts(0.01, 0)
    calls = {
        "gs_frame_backward": lambda g: _lib.gs_frame_backward(P(g), FAKE, *_grads(), None),
        "gs_frame_backward_part raster": lambda g: _lib.gs_frame_backward_part(P(g), FAKE, *_grads(), _lib.GS_BWD_RASTER, None),
        "gs_frame_backward_part geometry": lambda g: _lib.gs_frame_backward_part(P(g), None, *_grads(), _lib.GS_BWD_GEOMETRY, None),
        "gs_frame_backward_part color": lambda g: _lib.gs_frame_backward_part(P(g), None, *_grads(), _lib.GS_BWD_COLOR, None),
        "gs_frame_backward_slice": lambda g: _lib.gs_frame_backward_slice(P(g), *_grads(), _lib.GS_BWD_GEOMETRY, 0, 256, None),
        "gs_frame_backward_profile": lambda g: _lib.gs_frame_backward_profile(P(g), FAKE, *_grads(), ms3, None),
        "gs_frame_backward_adam": lambda g: _lib.gs_frame_backward_adam(P(g), FAKE, P(adam), None),
        "gs_frame_backward_adam_aux": lambda g: _lib.gs_frame_backward_adam_aux(P(g), FAKE, P(adam), None),
        "gs_frame_backward_adam_pose": lambda g: _lib.gs_frame_backward_adam_pose(P(g), FAKE, P(adam), None),
        "gs_frame_forward_project": lambda g: _lib.gs_frame_forward_project(P(g), 0, 1, None),
        "gs_frame_forward_rest": lambda g: _lib.gs_frame_forward_rest(P(g), None),
        "gs_frame_forward_profile": lambda g: _lib.gs_frame_forward_profile(P(g), ms6, None),
        "gs_frame_contrib": lambda g: _lib.gs_frame_contrib(P(g), P(opts), FAKE + (13 << 30), FAKE + (14 << 30), 1 << 30, None),
        "gs_frame_debug_views": lambda g: _lib.gs_frame_debug_views(P(g), *[P(p) for p in ptrs]),
    }
    for name, fn in calls.items():
        for g in (f, _frame(aux=True), _frame(pose=False)):
            assert fn(g) == GS_E_UNSUPPORTED, (name, _err())
            assert "GS_FRAME_DEVICE_POSE frames are not supported" in _err(), (name, _err())
    # the counter and overflow queries answer (these two return before any launch; the copies of the others are not issued here)
    ptr = C.c_void_p()
    assert _lib.gs_frame_overflow_flag(P(f), P(ptr)) == 0 and ptr.value
    assert _lib.gs_frame_debug_rects(P(f), P(ptr)) == 0 and ptr.value
    assert _lib.gs_frame_binning_variant(P(f)) == 2  # (1,000 Gaussians: the table variant)


# ------------------------------------------------------------------------------------------------------ refusals of gs_pose_*
STATE, LOG, GRAD, VALUES = FAKE + (15 << 30), FAKE + (16 << 30), FAKE + (17 << 30), FAKE + (17 << 30) + 64


def _opts(**kw):
    from gaussian import _lib

    o = _lib.GsPoseStepOpts(2e-3, 2e-3, 1.0, 0.9, 0.999, 1e-8, 1, 4)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _step(grad_rot=GRAD, grad_tran=GRAD + 36, values=VALUES, skip=None, opts=None, state=STATE, pose=POSE, log=LOG, log_rows=8,
          log_row=0):
    from gaussian import _lib

    o = _opts() if opts is None else opts
    return _lib.gs_pose_step(grad_rot, grad_tran, values, skip, C.byref(o) if o is not False else None, state, pose, log, log_rows,
                             log_row, None)


def test_pose_log_bytes():
    from gaussian import _lib

    q = _lib.gs_pose_log_bytes
    assert q(1, 4) == 4 * 28 and q(300, 4) == 300 * 4 * 28 and q(12, 8) == 12 * 4 * 32
    assert q(0, 4) == 0 and q(-1, 8) == 0 and q(5, 3) == 0 and q(5, 16) == 0


def test_pose_step_refusals():
    nan, inf = math.nan, math.inf
    bad = [dict(grad_rot=None), dict(grad_tran=None), dict(values=None), dict(opts=False), dict(state=None), dict(pose=None),
           dict(log=None),
           dict(opts=_opts(lr_rot=0.0)), dict(opts=_opts(lr_rot=-1e-3)), dict(opts=_opts(lr_tran=nan)), dict(opts=_opts(lr_tran=inf)),
           dict(opts=_opts(lr_scale=0.0)), dict(opts=_opts(lr_scale=nan)), dict(opts=_opts(eps=0.0)), dict(opts=_opts(eps=inf)),
           dict(opts=_opts(beta1=1.0)), dict(opts=_opts(beta1=-0.1)), dict(opts=_opts(beta2=1.0)), dict(opts=_opts(beta2=nan)),
           dict(opts=_opts(n_values=0)), dict(opts=_opts(n_values=5)), dict(opts=_opts(n_values=16)),
           dict(log_row=-1), dict(log_row=8), dict(log_rows=0),
           dict(state=STATE + 4), dict(pose=POSE + 8), dict(log=LOG + 4), dict(skip=FAKE + 4), dict(grad_rot=GRAD + 2),
           dict(values=VALUES + 1)]
    for kw in bad:
        assert _step(**kw) == GS_E_INVALID, kw
        assert _err().startswith("gs_pose_step: invalid argument"), (kw, _err())


def test_pose_reset_refusals():
    from gaussian import _lib

    eye = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    zero = (C.c_double * 3)(0, 0, 0)

    def reset(state=STATE, pose=POSE, log=LOG, log_rows=8, n_values=4, rot=eye, tran=zero):
        return _lib.gs_pose_reset(state, pose, log, log_rows, n_values, rot, tran, None)

    bad_rot = (C.c_double * 9)(1, 0, 0, 0, math.nan, 0, 0, 0, 1)
    bad_tran = (C.c_double * 3)(0, math.inf, 0)
    for kw in (dict(state=None), dict(pose=None), dict(log=None), dict(rot=None), dict(tran=None), dict(rot=bad_rot),
               dict(tran=bad_tran), dict(n_values=6), dict(log_rows=0), dict(state=STATE + 4), dict(pose=POSE + 4), dict(log=LOG + 8)):
        assert reset(**kw) == GS_E_INVALID, kw
        assert _err().startswith("gs_pose_reset: invalid argument"), (kw, _err())


# ------------------------------------------------------------------------------------------------------ the restatement
def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_follows_pose_adam_over_50_steps(seed):
    """Every entry of R, t, m, v within 1e-12 absolute after each of 50 consecutive steps on random gradients.  The arithmetic
    is some fifty double operations per step (about 1e-14 accumulated); a real mistake -- a transposed G R^T, a wrong bias
    correction, a wrong sign -- shows at 1e-3 or more."""
    from gs_track import PoseAdam

    rng = np.random.default_rng(seed)
    R0, t0 = _rotation(rng), rng.normal(size=3)
    total, lr_final = 50, 0.01
    adam = PoseAdam(R0, t0, 2e-3, 3e-3, (0.9, 0.999), 1e-8)
    st = pose_step_ref.new_state(R0, t0)
    worst = 0.0
    for k in range(total):
        scale = (10.0 ** rng.uniform(-3, 2)) if seed else 1.0  # (gradients of very different sizes from step to step)
        G = (rng.normal(size=9) * scale).astype(np.float32)
        gt = (rng.normal(size=3) * scale).astype(np.float32)
        if seed == 2 and k % 7 == 3:
            G[:] = 0.0  # (the rotation part of the step shrinks towards the series branch)
        lr_scale = lr_final ** (k / total)
        adam.step(G.astype(np.float64), gt.astype(np.float64), lr_scale)
        opts = pose_step_ref.default_opts(lr_rot=2e-3, lr_tran=3e-3, lr_scale=lr_scale)
        pose_step_ref.step(st, G, gt, [float(k), 0.0, 0.0, 0.0], opts, k)
        for got, want in ((st["R"], adam.rot.reshape(9)), (st["t"], adam.tran), (st["m"], adam.m), (st["v"], adam.v)):
            worst = max(worst, float(np.abs(np.array(got) - want).max()))
        assert st["steps"] == adam.k
    print(f"seed {seed}: largest |restatement - PoseAdam| over 50 steps = {worst:.3e}")
    assert worst <= 1e-12
    Rm = np.array(st["R"]).reshape(3, 3)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12


def test_restatement_small_angle_branch_and_bookkeeping():
    from gs_track import so3_exp

    for w in ((3e-9, -4e-9, 1e-9), (0.0, 0.0, 0.0), (1e-3, 2e-3, -5e-4), (0.7, -0.2, 1.1)):
        # (a dozen roundings of numbers up to 1.5 on either side: 1e-14 is five times that)
        assert np.abs(np.array(pose_step_ref.so3_exp(*w)).reshape(3, 3) - so3_exp(w)).max() <= 1e-14
    st = pose_step_ref.new_state(np.eye(3), np.zeros(3))
    before = {k: (list(v) if isinstance(v, list) else v) for k, v in st.items()}
    o = pose_step_ref.default_opts()
    g, t = [0.1, 0.2, -0.3, 0.4, 0.5, -0.6, 0.7, -0.8, 0.9], [0.2] * 3  # (G R^T not symmetric: the rotation moves)
    row = pose_step_ref.step(st, g, t, [1.0, 0, 0, 0], o, 0, skip=True)
    assert math.isnan(row[24]) and st["skipped"] == 1
    row = pose_step_ref.step(st, [math.nan] + g[1:], t, [1.0, 0, 0, 0], o, 1)
    row = pose_step_ref.step(st, g, t, [math.inf, 0, 0, 0], o, 2)
    assert st["bad"] == 2
    for k in ("R", "t", "m", "v", "best_R", "best_t", "best_loss", "steps", "best_row", "pose32"):
        assert st[k] == before[k], k
    pose_step_ref.step(st, g, t, [1.0, 0, 0, 0], pose_step_ref.default_opts(track_best=0), 3)
    assert st["steps"] == 1 and st["best_row"] == -1 and st["best_loss"] == math.inf
    pose_step_ref.step(st, g, t, [0.5, 0, 0, 0], o, 4)
    assert st["best_row"] == 4 and st["best_loss"] == 0.5 and st["best_R"] != st["R"]


def test_track_options_default_is_off_and_implies_pose_only():
    from gs_slam import SlamOptions
    from gs_track import TrackOptions, TrackResult

    assert TrackOptions().device_pose is False
    assert SlamOptions().track == TrackOptions()
    assert TrackOptions(device_pose=True) != TrackOptions()
    r = TrackResult(rot=np.eye(3), tran=np.zeros(3), loss=0.0, iterations=0)
    assert r.attempts == 1 and r.log is None


# ------------------------------------------------------------------------------------------------------ kernel resources
@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def _only(kernels, *parts):
    hits = [k for k in kernels if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits)
    return kernels[hits[0]]


TWINS = [(f"{base}_dp_kernelILb{b}E", f"{base}_kernelILb{b}E")
         for base in ("frame_project_count", "frame_project_count_pp", "frame_project_bin_count", "frame_project_bin_count_pp",
                      "frame_pose_backward") for b in (0, 1)]


def test_exactly_the_ten_twins_and_the_two_pose_kernels(kernels):
    assert len([k for k in kernels if "_dp_kernel" in k]) == len(TWINS) == 10
    assert len([k for k in kernels if "pose_step_kernel" in k or "pose_reset_kernel" in k]) == 2


@pytest.mark.parametrize("twin,by_value", TWINS, ids=[t[0] for t in TWINS])
def test_a_twin_needs_what_its_by_value_kernel_needs(kernels, twin, by_value):
    """No scratch, no VGPR spills; at most the by-value kernel's VGPRs + 4 and exactly its LDS and workgroup size.  (SGPRs
    parked in VGPR lanes are no scratch; the by-value project kernels park up to 16, and a twin may park no more than its own.)"""
    k, ref = _only(kernels, twin), _only(kernels, by_value)
    print(f"{twin}: {k['.vgpr_count']} VGPRs, {k['.sgpr_count']} SGPRs, {k['.group_segment_fixed_size']} bytes of LDS "
          f"(by value: {ref['.vgpr_count']} VGPRs, {ref['.sgpr_count']} SGPRs, {ref['.group_segment_fixed_size']} bytes)")
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
    assert k[".sgpr_spill_count"] <= ref[".sgpr_spill_count"]
    assert k[".vgpr_count"] <= ref[".vgpr_count"] + 4
    assert k[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == ref[".max_flat_workgroup_size"]


def test_pose_step_kernel_is_one_wave_without_scratch_or_lds(kernels):
    k = _only(kernels, "pose_step_kernel")
    print(f"pose_step_kernel: {k['.vgpr_count']} VGPRs, {k['.sgpr_count']} SGPRs")
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0
    assert k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 64
    r = _only(kernels, "pose_reset_kernel")
    assert r[".private_segment_fixed_size"] == 0 and r[".group_segment_fixed_size"] == 0
