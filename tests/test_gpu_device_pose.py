"""GPU tier of the device-resident pose (GS_FRAME_DEVICE_POSE, gs_pose_step; FrameRenderer.forward(pose_dev=...);
TrackOptions.device_pose; include/gs_abi.h):
  1. a flagged frame is the by-value frame of the pose its tensor holds, bit for bit, forward and backward -- whatever pose
     the descriptor carries --, and follows the tensor when it is overwritten;
  2. gs_pose_step against the Python restatement (tests/pose_step_ref.py) on gradients recorded from the host tracker;
  3. every frame of a device-pose ``track`` is the host path's frame at the logged pose, bit for bit;
  4. it tracks: the cases and thresholds of tests/test_gpu_track.py;
  5. nothing waits inside the loop, and a call whose workspace is too small is run again in a larger one."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pose_step_ref
from gaussian import _lib
from gs_frame import FrameRenderer
from gs_testutil import aux_case, to_torch
from gs_track import TrackOptions, Tracker
from track_ref import perturbed_start, pose_errors, so3_exp_series

pytestmark = pytest.mark.gpu

W_, H_ = 160, 120
GEOMETRY = _lib.GS_BWD_GEOMETRY


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _nan_pose(gpu):
    return (torch.full((3, 3), float("nan"), device=gpu), torch.full((3,), float("nan"), device=gpu))


def _pose12(cam, gpu):
    return torch.from_numpy(np.concatenate([np.asarray(cam.rot, np.float32).reshape(9),
                                            np.asarray(cam.tran, np.float32).reshape(3)])).to(gpu)


def _partial_rows(r, n, aux):
    """A copy of the pose workspace's partial rows (tests/test_gpu_pose_only.py)."""
    base = r._pose_ws.data_ptr()
    first = (base + 255) // 256 * 256 - base + 256
    rows = -(-n // 256) * (2 if aux else 1)
    return r._pose_ws[first:first + rows * 48].view(torch.float32).reshape(rows, 12).clone()


def _maps(gpu, aux, seed=5):
    gen = torch.Generator(gpu).manual_seed(seed)
    gimg = torch.randn(H_, W_, 3, device=gpu, generator=gen)
    gdep = torch.randn(H_, W_, device=gpu, generator=gen) * 0.1
    galp = torch.randn(H_, W_, device=gpu, generator=gen)
    return gimg, (dict(grad_depth=gdep, grad_alpha=galp) if aux else {})


def _frame_outputs(r, params, cam, aux, gimg, maps, pose_dev=None):
    """One forward and its pose backward -> every output, cloned: image, padded image, (depth, alpha, padded maps), the
    rectangle records, the pair counters, grad_rot / grad_tran and the partial rows of part 0 and of GS_BWD_GEOMETRY."""
    n = params[0].shape[0]
    out = r.forward(*params, cam, aux=aux, pose_dev=pose_dev)
    got = {"image": out[0].clone(), "padded": out[1].clone()}
    if aux:
        got["depth"], got["alpha"], got["aux_padded"] = out[2].clone(), out[3].clone(), r._aux_keep[2].clone()
    st = r.stats()
    got["counters"] = torch.tensor([st.visible, st.pairs, st.overflow])
    if n:
        got["rects"] = r._rects().clone()
    g0 = _nan_pose(r.device)
    r.backward_pose(gimg, g0, 0, **maps)
    got["grad_rot"], got["grad_tran"] = g0[0].clone(), g0[1].clone()
    if n:
        got["rows"] = _partial_rows(r, n, aux)
        r._pose_ws.fill_(0xFF)
    g1 = _nan_pose(r.device)
    r.backward_pose(None, g1, GEOMETRY)  # (from the rows part 0's raster backward left)
    got["grad_rot_geo"], got["grad_tran_geo"] = g1[0].clone(), g1[1].clone()
    if n:
        got["rows_geo"] = _partial_rows(r, n, aux)
    return got


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), (what, k, (a[k] != b[k]).nonzero().tolist()[:6])


def _flagged_equals_by_value(gpu, scene, cam, aux, r_kw=None, max_pairs=1 << 18, expect=None, leave_out=()):
    """The by-value frames at ``cam`` and at a second pose, then the flagged frames: the descriptor carries a THIRD pose
    throughout, the tensor first ``cam``'s, then -- overwritten in place -- the second's.  ``leave_out``: outputs not compared
    (the partial rows of an overflowed frame are sums over gradient rows nobody wrote: whatever each workspace held)."""
    params = to_torch(scene, gpu) if not isinstance(scene, list) else scene
    gimg, maps = _maps(gpu, aux)
    kw = dict(max_pairs=max_pairs, training=True, auto_grow=False, **(r_kw or {}))
    cam2 = copy.copy(cam)
    cam2.rot = (so3_exp_series(np.array([0.004, -0.006, 0.003])) @ cam.rot.astype(np.float64)).astype(np.float32)
    cam2.tran = (cam.tran.astype(np.float64) + np.array([0.01, 0.004, -0.008])).astype(np.float32)
    decoy = copy.copy(cam)
    decoy.rot = (so3_exp_series(np.array([-0.3, 0.2, 0.1])) @ cam.rot.astype(np.float64)).astype(np.float32)
    decoy.tran = (cam.tran.astype(np.float64) + np.array([-0.2, 0.1, 0.3])).astype(np.float32)
    r = FrameRenderer(gpu, **kw)

    def outputs(*a, **k):
        got = _frame_outputs(*a, **k)
        return {name: v for name, v in got.items() if name not in leave_out}

    want = [outputs(r, params, c, aux, gimg, maps) for c in (cam, cam2)]
    if expect is not None:
        assert r.binning_variant() == expect
    rd = FrameRenderer(gpu, **kw)
    pose = _pose12(cam, gpu)
    got = outputs(rd, params, decoy, aux, gimg, maps, pose_dev=pose)
    assert rd._frame.flags & _lib.GS_FRAME_DEVICE_POSE
    if expect is not None:
        assert rd.binning_variant() == expect
    _assert_same(got, want[0], "flagged frame vs by-value frame")
    pose.copy_(_pose12(cam2, gpu))
    got2 = outputs(rd, params, decoy, aux, gimg, maps, pose_dev=pose)
    _assert_same(got2, want[1], "flagged frame after its pose tensor was overwritten")
    return want


def _live(want):
    """The two by-value frames differ (the second pose is another frame) and have something to differentiate."""
    a, b = want
    assert not _same_bits(a["image"], b["image"]) and not _same_bits(a["grad_rot"], b["grad_rot"])
    assert int(a["counters"][1]) > 0 and int(a["counters"][2]) == 0
    assert torch.isfinite(a["grad_rot"]).all() and float(a["grad_rot"].abs().max()) > 0 and float(a["grad_tran"].abs().max()) > 0
    assert _same_bits(a["grad_rot"], a["grad_rot_geo"]) and _same_bits(a["rows"], a["rows_geo"])


# ------------------------------------------------------------------------------------------- 1. a flagged frame is the frame
@pytest.mark.parametrize("variant", ["table", "strip"])
@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("n", [37, 6_000, 6_001])
def test_flagged_frame_equals_the_by_value_frame(gpu, n, aux, variant):
    scene, cam = aux_case(n, W_, H_, seed=11, yaw=3.0)
    _live(_flagged_equals_by_value(gpu, scene, cam, aux, r_kw=dict(force_strips=variant == "strip"), expect=variant))


@pytest.mark.parametrize("variant", ["table", "strip"])
@pytest.mark.parametrize("case", ["offcentre", "dist"])
def test_flagged_frame_off_centre_and_dist_listing(gpu, case, variant):
    """The *_pp twins (an off-centre principal point) and the DIST instantiations, aux frames of 6,001 Gaussians."""
    scene, cam = aux_case(6_001, W_, H_, seed=11, yaw=3.0)
    r_kw = dict(force_strips=variant == "strip")
    if case == "offcentre":
        cam.cx, cam.cy = W_ / 2 + 7.25, H_ / 2 - 4.5
    else:
        r_kw.update(tile_culling_method="dist", tile_culling_dist_thresh=0.5)
    want = _flagged_equals_by_value(gpu, scene, cam, True, r_kw=r_kw, expect=variant)
    _live(want)


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
def test_flagged_frame_overflowed_and_empty(gpu, aux):
    """A pair capacity far too small (the frame is rendered empty, the pose gradient is zeros) and N = 0: the same on both
    paths."""
    scene, cam = aux_case(4_000, W_, H_, seed=4)
    want = _flagged_equals_by_value(gpu, scene, cam, aux, max_pairs=64, leave_out=("rows", "rows_geo"))
    assert int(want[0]["counters"][2]) > 0 and not want[0]["grad_rot"].any() and not want[0]["grad_tran"].any()
    empty = [torch.zeros(*s, device=gpu) for s in ((0, 3), (0, 4), (0, 3), (0,), (0, 3))]
    want = _flagged_equals_by_value(gpu, empty, cam, aux, max_pairs=1 << 12)
    assert not want[0]["grad_rot"].any() and not want[0]["image"].any()


def test_renderer_refusals(gpu):
    scene, cam = aux_case(500, W_, H_, seed=3)
    params = to_torch(scene, gpu)
    pose = _pose12(cam, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 16, training=True, auto_grow=False)
    with pytest.raises(RuntimeError, match="pose_dev must hold 12 floats"):
        r.forward(*params, cam, pose_dev=pose[:9])
    with pytest.raises(RuntimeError, match="pose_dev must be a contiguous float32 HIP tensor"):
        r.forward(*params, cam, pose_dev=pose.double())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        r.forward(*params, cam, pose_dev=torch.zeros(16, device=gpu)[1:13])
    with pytest.raises(RuntimeError, match="needs a training frame"):
        r.forward(*params, cam, training=False, pose_dev=pose)
    with pytest.raises(RuntimeError, match="needs rgb colours"):
        r.forward(*params[:4], torch.zeros(500, 27, device=gpu), cam, pose_dev=pose)
    with pytest.raises(RuntimeError, match="sort_mode 2"):
        FrameRenderer(gpu, max_pairs=1 << 16, training=True, auto_grow=False, sort_mode=1).forward(*params, cam, pose_dev=pose)
    r.forward(*params, cam, pose_dev=pose)
    gimg = torch.ones(H_, W_, 3, device=gpu)
    with pytest.raises(RuntimeError, match="GS_FRAME_DEVICE_POSE frames are not supported"):
        r.backward(gimg)  # (the library's refusal: nothing was enqueued)
    with pytest.raises(RuntimeError, match="must be the tensor the frame's forward was given"):
        r.backward_pose(gimg, _nan_pose(gpu), pose_dev=pose.clone())
    gp = _nan_pose(gpu)
    r.backward_pose(gimg, gp, pose_dev=pose)
    assert torch.isfinite(gp[0]).all()


# ------------------------------------------------------------------------------------------- the tracking scene, built once
_SCENE = {}


def _scene(gpu):
    """The scene of tests/test_gpu_track.py, a renderer for targets, its target at the true pose and the perturbed start."""
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True, occlusion_cull=False)
        _SCENE["x"] = (params, cam, r)
        img, rng = _target(gpu, cam.rot, cam.tran)
        start = perturbed_start(cam.rot.astype(np.float64), cam.tran.astype(np.float64))
        _SCENE["y"] = (img.clone(), rng.clone(), start)
    return _SCENE["x"] + _SCENE["y"]


def _target(gpu, rot, tran):
    params, cam, r = _SCENE["x"]
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    img, _, d, a = r.forward(*params, c, training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
    return img.contiguous(), rng.contiguous()


def _variant_options(variant, **kw):
    kw.setdefault("iterations", 12)
    if variant == "median_gate":
        kw["depth_gate_k"] = 10.0
    if variant == "pyramid":
        kw["pyramid"] = ((1, 6), (0, 6))
    return kw


# ------------------------------------------------------------------------------------------- 2. gs_pose_step vs the restatement
def _read_state(buf):
    return _lib.GsPoseState.from_buffer_copy(buf.cpu().numpy().tobytes()[:C.sizeof(_lib.GsPoseState)])


def _state_arrays(s):
    return {k: np.array(getattr(s, k), np.float64) for k in ("R", "t", "m", "v", "best_R", "best_t")}


def test_pose_step_follows_the_restatement_on_recorded_gradients(gpu):
    """12 iterations of the host tracker recorded (gradients, values), then replayed through gs_pose_step and through
    tests/pose_step_ref.py: the double state within the CPU tier's 1e-12 after every step, pose_dev the fp32 of the device's
    own state bit for bit, the log rows exact; a set skip flag and a NaN gradient change nothing but their counters, and
    track_best = 0 never touches ``best``."""
    params, cam, _, img, rng, (R0, t0) = _scene(gpu)
    total, o = 12, TrackOptions(pose_only=True)
    host = Tracker(params, cam, o, gpu)
    from gs_track import PoseAdam

    adam, R, t, recorded = PoseAdam(R0, t0, o.lr_rot, o.lr_tran, o.betas, o.eps), R0, t0, []
    for k in range(total):
        h = host.iteration(R, t, img, rng).numpy().copy()
        recorded.append(h)
        R, t = adam.step(h[0:9].astype(np.float64), h[9:12].astype(np.float64), o.lr_final ** (k / total))
    rows, nv = total + 4, 4
    state_dev = torch.zeros(C.sizeof(_lib.GsPoseState), dtype=torch.uint8, device=gpu)
    pose, log = torch.zeros(12, device=gpu), torch.full((rows, 24 + nv), float("nan"), device=gpu)
    flag = torch.zeros(1, dtype=torch.int64, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("gs_pose_reset", state_dev.data_ptr(), pose.data_ptr(), log.data_ptr(), rows, nv,
              (C.c_double * 9)(*R0.reshape(9)), (C.c_double * 3)(*t0), stream)
    assert not log.any()  # zeroed
    ref = pose_step_ref.new_state(R0.reshape(9), t0)
    assert pose.cpu().tolist() == ref["pose32"]

    def step(k, h, track_best=1, skip=False):
        g = torch.from_numpy(h).to(gpu)
        opts = _lib.GsPoseStepOpts(o.lr_rot, o.lr_tran, o.lr_final ** (min(k, total - 1) / total), o.betas[0], o.betas[1], o.eps,
                                   track_best, nv)
        flag.fill_(7 if skip else 0)
        _lib.call("gs_pose_step", g[0:9].data_ptr(), g[9:12].data_ptr(), g[12:16].data_ptr(), flag.data_ptr(), C.byref(opts),
                  state_dev.data_ptr(), pose.data_ptr(), log.data_ptr(), rows, k, stream)
        ro = pose_step_ref.default_opts(lr_rot=o.lr_rot, lr_tran=o.lr_tran, lr_scale=opts.lr_scale, beta1=o.betas[0],
                                        beta2=o.betas[1], eps=o.eps, track_best=track_best, n_values=nv)
        row = pose_step_ref.step(ref, h[0:9].tolist(), h[9:12].tolist(), h[12:16].tolist(), ro, k, skip=skip)
        got = log[k].cpu().numpy()
        want = np.array(row, np.float32)
        nan = np.isnan(want)  # (a skipped row's loss, a bad row's input)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), k
        return _read_state(state_dev)

    worst = 0.0
    for k, h in enumerate(recorded):
        s = step(k, h, track_best=int(k >= 4))  # (the first four rows do not compete: as the coarse stage of a schedule)
        dev = _state_arrays(s)
        for name in dev:
            worst = max(worst, float(np.abs(dev[name] - np.array(ref[name])).max()))
        assert (s.steps, s.best_row, s.skipped, s.bad) == (ref["steps"], ref["best_row"], 0, 0)
        assert s.best_loss == ref["best_loss"]
        if k < 4:
            assert s.best_row == -1 and math.isinf(s.best_loss) and np.array_equal(dev["best_R"], R0.reshape(9))
        # pose_dev: the device's own double state rounded to fp32 once
        assert np.array_equal(pose.cpu().numpy(), np.concatenate([dev["R"], dev["t"]]).astype(np.float32))
    print(f"gs_pose_step vs restatement over {total} recorded steps: largest |difference| = {worst:.3e}")
    assert worst <= 1e-12
    assert ref["best_row"] >= 4
    # the host's own optimizer got to the same place
    assert np.abs(np.array(ref["R"]).reshape(3, 3) - R).max() <= 1e-12 and np.abs(np.array(ref["t"]) - t).max() <= 1e-12
    # a set skip flag, a NaN gradient, a non-finite loss: R, t, m, v, best and pose_dev keep their bits
    before, pose_before = bytes(state_dev.cpu().numpy().tobytes()[:37 * 8]), pose.clone()
    s = step(total, recorded[3], skip=True)
    assert (s.skipped, s.bad, s.steps) == (1, 0, total)
    bad = recorded[5].copy()
    bad[4] = np.nan
    s = step(total + 1, bad)
    bad = recorded[5].copy()
    bad[9] = np.inf
    s = step(total + 2, bad)
    bad = recorded[5].copy()
    bad[12] = np.nan
    s = step(total + 3, bad)
    assert (s.skipped, s.bad, s.steps) == (1, 3, total)
    assert bytes(state_dev.cpu().numpy().tobytes()[:37 * 8]) == before and _same_bits(pose, pose_before)


# ------------------------------------------------------------------------------------------- 3. the loop's frames
@pytest.mark.parametrize("variant", ["rgb", "rgbd", "median_gate", "pyramid"])
def test_every_frame_of_the_loop_is_the_host_paths_frame(gpu, variant):
    params, cam, _, img, rng, start = _scene(gpu)
    before = [p.clone() for p in params]
    kw = _variant_options(variant)
    target_rng = None if variant == "rgb" else rng
    dev = Tracker(params, cam, TrackOptions(device_pose=True, **kw), gpu)
    assert dev.opt.pose_only and dev._scratch is None and dev.renderer.auto_grow is False
    res = dev.track(img, target_rng, init=start)
    assert res.attempts == 1 and res.iterations == 12 == len(res.losses) == res.log.shape[0]
    host = Tracker(params, cam, TrackOptions(pose_only=True, **kw), gpu)
    if variant == "pyramid":
        images, ranges = host._pyramid.build(img, target_rng)
        levels = [lv for lv, _, n in res.levels for _ in range(n)]
        assert res.levels == [(1, 0, 6), (0, 6, 6)]
    else:
        images, ranges, levels = {0: img}, {0: target_rng}, [0] * 12
        assert res.levels is None
    nv = res.log.shape[1] - 24
    assert nv == (8 if variant == "median_gate" else 4)
    ref = pose_step_ref.new_state(start[0].reshape(9), start[1])
    total = 12
    for k in range(total):
        row = res.log[k]
        # the row's pose is the pose the step before left in pose_dev: fp32 of a double within 1e-12 of the restatement's
        want = np.array(ref["R"] + ref["t"])
        assert np.abs(row[0:12].astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-12, k
        if k == 0:
            assert row[0:12].tolist() == ref["pose32"]
        lv = levels[k]
        h = host.iteration(row[0:9].astype(np.float64).reshape(3, 3), row[9:12].astype(np.float64), images[lv],
                           None if ranges[lv] is None else ranges[lv], lv).numpy()
        assert np.array_equal(h[0:12].view(np.int32), row[12:24].view(np.int32)), (k, h[0:12], row[12:24])
        assert np.array_equal(h[12:12 + nv].view(np.int32), row[24:24 + nv].view(np.int32)), (k, h[12:], row[24:])
        assert res.losses[k] == float(h[12])
        o = dev.opt
        ro = pose_step_ref.default_opts(lr_rot=o.lr_rot, lr_tran=o.lr_tran, lr_scale=o.lr_final ** (k / total), beta1=o.betas[0],
                                        beta2=o.betas[1], eps=o.eps, track_best=int(lv == levels[-1]), n_values=nv)
        pose_step_ref.step(ref, row[12:21].tolist(), row[21:24].tolist(), row[24:24 + nv].tolist(), ro, k)
    # what came back: the best of the last stage's rows, the pose that row rendered (to the restatement's 1e-12)
    last = [k for k in range(total) if levels[k] == levels[-1]]
    assert res.loss == min(res.losses[k] for k in last) == ref["best_loss"]
    assert np.abs(res.rot.reshape(9) - np.array(ref["best_R"])).max() <= 1e-12
    assert np.abs(res.tran - np.array(ref["best_t"])).max() <= 1e-12
    if variant == "median_gate":
        g = res.log[ref["best_row"], 27:32]
        assert res.inliers == (int(g[0]), int(g[4]), int(g[1])) and res.medians == (float(g[2]), float(g[3]))
        assert res.inliers[0] > 0 and res.medians[0] > 0
    else:
        assert res.inliers is None and res.medians is None
    for p, k in zip(params, before):
        assert torch.equal(p, k)


# ------------------------------------------------------------------------------------------- 4. it tracks
@pytest.mark.parametrize("with_depth", [False, True])
def test_device_pose_tracker_recovers_a_single_frame(gpu, with_depth):
    """tests/test_gpu_track.py::test_tracker_recovers_a_single_frame with device_pose=True: its case, its thresholds."""
    params, cam, _, img, rng, (R0, t0) = _scene(gpu)
    before = [p.clone() for p in params]
    R_true, t_true = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    e_r0, e_t0 = pose_errors(R0, t0, R_true, t_true)
    tr = Tracker(params, cam, TrackOptions(device_pose=True), gpu)
    res = tr.track(img, rng if with_depth else None, init=(R0, t0))
    e_r, e_t = pose_errors(res.rot, res.tran, R_true, t_true)
    print(f"device-pose tracker single frame depth={with_depth}: rot {e_r0:.3e} -> {e_r:.3e}, tran {e_t0:.3e} -> {e_t:.3e}, "
          f"loss {res.losses[0]:.5f} -> {res.loss:.6f}, attempts {res.attempts}")
    assert abs(e_r0 - math.radians(0.5)) < 1e-4 and abs(e_t0 - 0.02) < 1e-9
    assert e_r <= 0.1 * e_r0 and e_t <= 0.1 * e_t0, (e_r0, e_r, e_t0, e_t)
    for a, b in zip(before, params):
        assert torch.equal(a, b) and a.grad is None and b.grad is None
    assert res.iterations == 300 == len(res.losses) and res.loss == min(res.losses)
    assert np.abs(res.rot @ res.rot.T - np.eye(3)).max() <= 1e-6
    again = float(tr.iteration(res.rot, res.tran, img, rng if with_depth else None)[12])
    assert again == res.loss


def test_device_pose_tracker_follows_a_sequence(gpu):
    """tests/test_gpu_track.py::test_tracker_follows_a_sequence with device_pose=True: its poses, its thresholds."""
    params, cam, _, _, _, _ = _scene(gpu)
    rng_ = np.random.default_rng(211)
    axis = rng_.normal(size=3)
    axis /= np.linalg.norm(axis)
    dR = so3_exp_series(axis * math.radians(0.5))
    u = rng_.normal(size=3)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * 0.02 - (dR @ t - t)
    poses = [(R, t)]
    for _ in range(5):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    motion = [None] + [pose_errors(*poses[k], *poses[k - 1]) for k in range(1, 6)]
    tr = Tracker(params, cam, TrackOptions(device_pose=True), gpu)
    errs = []
    for R, t in poses:
        img, rng = _target(gpu, R, t)
        res = tr.track(img, rng)
        errs.append(pose_errors(res.rot, res.tran, R, t))
    print("device-pose tracker sequence: errors after tracking " + ", ".join(f"({a:.2e}, {b:.2e})" for a, b in errs))
    for k in range(1, 6):
        assert abs(motion[k][0] - math.radians(0.5)) < 1e-4 and abs(motion[k][1] - 0.02) < 0.02 * 0.02
    for k in range(2, 6):
        assert errs[k][0] <= 0.1 * motion[k][0] and errs[k][1] <= 0.1 * motion[k][1], (k, errs)


# ------------------------------------------------------------------------------------------- 5. no waiting inside the loop
class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def _count_copies(t):
    """Wrap ``t.copy_`` (an instance attribute shadows the method) -> the counter."""
    c = _Counted(t.copy_)
    t.copy_ = c
    return c


def test_nothing_waits_inside_the_loop_and_a_small_workspace_is_grown(gpu, monkeypatch):
    params, cam, _, img, rng, start = _scene(gpu)
    iterations = _Counted(Tracker.iteration)
    monkeypatch.setattr(Tracker, "iteration", lambda self, *a, **kw: iterations(self, *a, **kw))
    results = {}
    for name, max_pairs in (("large", 1 << 20), ("small", 4096)):
        tr = Tracker(params, cam, TrackOptions(device_pose=True, iterations=12, max_pairs=max_pairs), gpu)
        reads, host_path = _count_copies(tr._dp["host"]), _count_copies(tr._host)
        stats = _Counted(tr.renderer.stats)
        tr.renderer.stats = stats
        res = results[name] = tr.track(img, rng, init=start)
        assert iterations.calls == 0 and host_path.calls == 0
        assert reads.calls == res.attempts
        # the renderer's counters are read only between attempts, to size the next one
        assert stats.calls == res.attempts - 1
        assert not np.isnan(res.losses).any() and res.iterations == 12
    assert results["large"].attempts == 1 and 2 <= results["small"].attempts <= 3
    a, b = results["large"], results["small"]
    assert np.array_equal(a.rot, b.rot) and np.array_equal(a.tran, b.tran) and a.loss == b.loss and a.losses == b.losses
