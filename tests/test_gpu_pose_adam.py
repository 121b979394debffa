"""GPU tier of the fused training step with a pose gradient (gs_frame_backward_adam_pose, include/gs_abi.h) and of what is
built on it: FrameRenderer.backward_adam(grad_pose=...) bit for bit against backward(grad_pose=...) + FusedAdam.step() --
parameters, moments, statistic AND the pose gradient --, the pose gradient against the per-Gaussian gradients, the Trainer's
free poses, a joint fit of poses and map that has to recover perturbed poses, and gs_slam.Slam with refine_poses on the
eight-frame arc of tests/test_gpu_slam.py (whose helpers are restated here).  The figures the last two print belong in
profiles/pose_refine.txt."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_dp import FlatGaussianParams
from gs_frame import FrameRenderer
from gs_scene import make_camera, make_scene
from gs_testutil import aux_case, to_torch
from gs_train import FusedAdam, TrainOptions, Trainer, base_lrs
from track_ref import pose_errors, so3_exp_series

pytestmark = pytest.mark.gpu

GS_PB_BIG = 64  # frame_project_backward_body.inc: rows beyond which the whole workgroup sums an rgb Gaussian
NT_MIN_N = -(-(300 << 20) // (14 * 16))  # project_bwd.hip: N (11 + 3) 16 bytes > 300 MiB takes the non-temporal instantiation


def _nan_pose(gpu):
    return (torch.full((3, 3), float("nan"), device=gpu), torch.full((3,), float("nan"), device=gpu))


# ------------------------------------------------------------------------------- a. fused = unfused, bit for bit, pose too
def _pose_pair(gpu, scene, cam, kind, stat, steps, max_pairs=1 << 20, seed=5, probe=None, auto_grow=True, momentum=None):
    """`steps` optimizer steps from identical copies through backward_adam(grad_pose) and through backward(grad_pose) +
    FusedAdam.step, random dL/dimage (None for kind "aux_noimage"), dL/ddepth, dL/dalpha per step.
    -> the two end states [(flat parameters, exp_avg, exp_avg_sq, statistic, [(grad_rot, grad_tran) per step])]."""
    H, W = cam.height, cam.width
    aux = kind != "plain"
    start = to_torch(scene, gpu)
    lrs = [b * 0.5 for b in base_lrs(TrainOptions())]
    out = []
    for fuse in (True, False):
        gen = torch.Generator(gpu).manual_seed(seed)
        flat = FlatGaussianParams([t.clone() for t in start])
        opt = FusedAdam(flat, lrs, grad_stat=stat)
        if momentum is not None:
            opt.exp_avg.fill_(momentum)
        r = FrameRenderer(gpu, max_pairs=max_pairs, training=True, auto_grow=auto_grow)
        poses = []
        for _ in range(steps):
            r.forward(*flat.params, cam, aux=aux)
            if auto_grow:
                assert not r.last_frame_overflowed(wait=True)
            if probe is not None:
                probe(r)
            gimg = torch.randn(H, W, 3, device=gpu, generator=gen) if kind != "aux_noimage" else None
            gdep = torch.randn(H, W, device=gpu, generator=gen) * 0.1
            galp = torch.randn(H, W, device=gpu, generator=gen)
            maps = dict(grad_depth=gdep, grad_alpha=galp) if aux else {}
            opt.skip_flag = r.overflow_flag()
            gp = _nan_pose(gpu)
            if fuse:
                r.backward_adam(gimg, opt.fused_descriptor(), grad_pose=gp, **maps)
            else:
                r.backward(gimg, out=flat.grads, grad_pose=gp, **maps)
                opt.step()
            poses.append(gp)
        assert opt.step_count == steps
        out.append((flat.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(),
                    opt.accum_grad.clone() if opt.accum_grad is not None else torch.zeros(1, device=gpu), poses))
        del r, opt, flat
        torch.cuda.empty_cache()
    return out


def _assert_same(got, stat, moved=True):
    """All five parameter arrays (the flat buffer), all ten moments (the two flat moment buffers), grad_stat, and every step's
    grad_rot and grad_tran."""
    for a, b, name in zip(got[0][:4], got[1][:4], ("parameters", "exp_avg", "exp_avg_sq", "grad statistic")):
        assert torch.equal(a, b), name
    assert len(got[0][4]) == len(got[1][4]) > 0
    for k, (a, b) in enumerate(zip(got[0][4], got[1][4])):
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all(), k
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
    if moved:
        assert float(got[0][1].abs().max()) > 0
        assert all(float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0 for a in got[0][4])
        if stat is not None:
            assert float(got[0][3].abs().max()) > 0


@pytest.mark.parametrize("stat", [None, "max", "mean"])
@pytest.mark.parametrize("n", [37, 6_000, 6_001])
@pytest.mark.parametrize("kind", ["plain", "aux", "aux_noimage"])
def test_fused_pose_step_equals_backward_then_adam(gpu, kind, n, stat):
    """One partial wave; 6,000; 6,001 (a ragged float4 end, N no multiple of 256) -- statistic modes 0 / 1 / 2 -- plain frames,
    aux frames with all three gradients, aux frames with dL/dimage = None."""
    W, H = 160, 112
    got = _pose_pair(gpu, make_scene(n, W, H, seed=11), make_camera(W, H, yaw_deg=3.0), kind, stat, steps=3)
    _assert_same(got, stat)


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_fused_pose_step_with_workgroup_summed_and_culled_gaussians(gpu, kind):
    """Gaussians beyond GS_PB_BIG tiles (summed by the whole workgroup before the epilogue) and Gaussians the frustum culls
    (zero pose terms, a zero-gradient step) in the same frame -- both asserted from the rectangle records."""
    W, H = 192, 128
    scene, cam = aux_case(8_000, W, H, seed=47, yaw=8.0, max_px_sigma=48.0)
    seen = []

    def probe(r):
        rc = r._rects()
        seen.append((int(((rc[:, 2] != 0) & (rc[:, 3] > GS_PB_BIG)).sum()), int((rc[:, 2] == 0).sum())))

    got = _pose_pair(gpu, scene, cam, kind, "max", steps=3, probe=probe)
    assert min(b for b, _ in seen) > 0 and min(c for _, c in seen) > 0, seen
    _assert_same(got, "max")


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_fused_pose_step_non_temporal_instantiation(gpu, kind):
    """The smallest N whose 14 parameters x 16 bytes exceed 300 MiB (the ADAM = 2 instantiations), on a small image."""
    n, W, H = NT_MIN_N, 160, 112
    assert n == 1_404_343 and n * 14 * 16 > (300 << 20) >= (n - 1) * 14 * 16
    got = _pose_pair(gpu, make_scene(n, W, H, seed=13, max_px_sigma=3.0), make_camera(W, H, yaw_deg=3.0), kind, "max",
                     steps=2, max_pairs=1 << 23)
    _assert_same(got, "max")


@pytest.mark.parametrize("kind", ["plain", "aux"])
def test_fused_pose_step_skips_overflowed_frames(gpu, kind):
    """A pair capacity far too small: the frame is rendered empty, no step is taken (momentum that WOULD move the parameters
    is in place), and grad_rot / grad_tran are exactly zero -- on both paths."""
    W, H = 128, 96
    scene, cam = make_scene(4_000, W, H, seed=4), make_camera(W, H)
    start = FlatGaussianParams([t.clone() for t in to_torch(scene, gpu)]).flat_param.clone()
    got = _pose_pair(gpu, scene, cam, kind, "max", steps=1, max_pairs=64, auto_grow=False, momentum=0.5)
    _assert_same(got, "max", moved=False)
    flat, m, v, stat_, poses = got[0]
    assert torch.equal(flat, start)
    assert float((m - 0.5).abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and float(stat_.abs().max()) == 0.0
    assert torch.equal(poses[0][0], torch.zeros(3, 3, device=gpu)) and torch.equal(poses[0][1], torch.zeros(3, device=gpu))


def test_fused_pose_step_of_an_empty_frame_writes_zeros(gpu):
    """N = 0: no kernel runs, the pose gradient is written (zeros) all the same."""
    cam = make_camera(128, 96)
    z = lambda *s: torch.zeros(*s, device=gpu, dtype=torch.float32)  # noqa: E731
    params = (z(0, 3), z(0, 4), z(0, 3), z(0), z(0, 3))
    dummy = z(64)  # (moments of N = 0 Gaussians: never touched, but not NULL)
    r = FrameRenderer(gpu, max_pairs=1 << 12, training=True, auto_grow=False)
    adam = _lib.GsAdamFused()
    for k in range(5):
        adam.exp_avg[k] = adam.exp_avg_sq[k] = dummy.data_ptr()
        adam.lr[k] = 1e-3
    adam.beta1, adam.beta2, adam.eps, adam.step = 0.9, 0.99, 1e-8, 1
    for aux in (False, True):
        image, *_ = r.forward(*params, cam, aux=aux)
        gp = _nan_pose(gpu)
        f = r._pose_frame(r._frame, gp, 0)
        with torch.cuda.device(gpu):
            _lib.check(_lib.gs_frame_backward_adam_pose(ctypes.byref(f), torch.ones_like(image).data_ptr(), ctypes.byref(adam),
                                                        torch.cuda.current_stream(gpu).cuda_stream),
                       "gs_frame_backward_adam_pose")
        assert torch.equal(gp[0], z(3, 3)) and torch.equal(gp[1], z(3))
    assert float(dummy.abs().max()) == 0.0


# ------------------------------------------------------------------------------- b. the pose gradient is the right one
def test_fused_pose_gradient_satisfies_the_translation_identity(gpu):
    """dL/dtran = rot . sum_i dL/dpos_i (tests/test_gpu_pose.py::_check_identities, its tolerance), the per-Gaussian gradients
    from the unfused backward of the same frame; and the fused call's pose gradient is that backward's, bit for bit."""
    W, H = 160, 112
    scene, cam = make_scene(6_000, W, H, seed=11), make_camera(W, H, yaw_deg=3.0)
    g = torch.Generator(gpu).manual_seed(17)
    gimg, gdep, galp = (torch.randn(H, W, 3, device=gpu, generator=g), torch.randn(H, W, device=gpu, generator=g) * 0.1,
                        torch.randn(H, W, device=gpu, generator=g))
    maps = dict(grad_depth=gdep, grad_alpha=galp)
    p_ref = to_torch(scene, gpu)
    r_ref = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=True)
    r_ref.forward(*p_ref, cam, aux=True)
    gp_ref = _nan_pose(gpu)
    grads = r_ref.backward(gimg, grad_pose=gp_ref, **maps)
    flat = FlatGaussianParams([t.clone() for t in p_ref])
    opt = FusedAdam(flat, base_lrs(TrainOptions()), grad_stat=None)
    r = FrameRenderer(gpu, max_pairs=1 << 20, training=True, auto_grow=True)
    r.forward(*flat.params, cam, aux=True)
    gp = _nan_pose(gpu)
    r.backward_adam(gimg, opt.fused_descriptor(), grad_pose=gp, **maps)
    assert torch.equal(gp[0], gp_ref[0]) and torch.equal(gp[1], gp_ref[1])
    assert not torch.equal(flat.params[0], p_ref[0])  # (the step was taken: the gradient is the pre-step frame's)
    R = torch.as_tensor(np.asarray(cam.rot, np.float64), device=gpu)
    terms = grads[0].double() @ R.T
    lhs, rhs, mag = gp[1].double(), terms.sum(0), terms.abs().sum(0)
    print("translation identity: |lhs - rhs| / mag =", ((lhs - rhs).abs() / mag).tolist())
    assert torch.all((lhs - rhs).abs() <= 1e-5 * mag + 1e-30), (lhs, rhs, mag)
    assert float(lhs.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------- c. refusals
def test_backward_adam_with_a_pose_refuses_sh_renderers(gpu):
    W, H = 128, 96
    scene, cam = aux_case(3_000, W, H, seed=101, use_sh=True)
    flat = FlatGaussianParams([t.clone() for t in to_torch(scene, gpu)])
    opt = FusedAdam(flat, base_lrs(TrainOptions()))
    r = FrameRenderer(gpu, max_pairs=1 << 18, training=True, auto_grow=True)
    before = flat.flat_param.clone()
    for aux in (False, True):
        r.forward(*flat.params, cam, aux=aux)
        with pytest.raises(RuntimeError, match="rgb colours"):
            r.backward_adam(torch.ones(H, W, 3, device=gpu), opt.fused_descriptor(advance=False), grad_pose=_nan_pose(gpu))
    assert torch.equal(flat.flat_param, before)
    tr = Trainer([t.clone() for t in to_torch(scene, gpu)], [cam], [torch.zeros(H, W, 3, device=gpu)], TrainOptions())
    from gs_track import _SH_REFUSAL

    with pytest.raises(RuntimeError) as e:
        tr.free_pose(0, 1e-3, 1e-3)
    assert str(e.value) == _SH_REFUSAL


# ------------------------------------------------------------------------------------------------------------ d. Trainer
def _truth(gpu, scene, cams):
    """Truth images and truth range maps (depth / alpha where alpha >= 0.5, else 0 = no measurement) of `cams`
    (tests/test_gpu_rgbd.py)."""
    gt = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 20, auto_grow=True)
    images, ranges = [], []
    for cam in cams:
        img, _, d, a = r.forward(*gt, cam, training=False, aux=True)
        images.append(img.clone())
        ranges.append(torch.where(a >= 0.5, d / a.clamp_min(1e-6), torch.zeros_like(d)).contiguous())
    return images, ranges


def _cams(W, H, shifts):
    out = []
    for yaw, tx in shifts:
        c = make_camera(W, H, yaw_deg=yaw)
        c.tran = np.array([tx, 0.0, 0.0], np.float32)
        out.append(c)
    return out


class _Calls:
    """Counts the calls of gs_frame_backward_adam_pose through a wrapper on `_lib`."""

    def __enter__(self):
        self.n, self._orig = 0, _lib.gs_frame_backward_adam_pose

        def wrapper(*a):
            self.n += 1
            return self._orig(*a)

        _lib.gs_frame_backward_adam_pose = wrapper
        return self

    def __exit__(self, *exc):
        _lib.gs_frame_backward_adam_pose = self._orig


@pytest.mark.parametrize("rgbd", [False, True])
def test_trainer_with_frozen_rates_is_the_trainer_without_free_poses(gpu, rgbd):
    """free_pose(i, 0, 0) on every view: 12 steps over three views go through the new entry point and leave parameters and
    moments equal, bit for bit, to those of a Trainer that never freed a pose (which never calls it); the poses and the
    caller's cameras stay what they were."""
    W, H = 160, 112
    scene = make_scene(6_000, W, H, seed=11)
    cams = _cams(W, H, [(-3.0, -0.05), (0.0, 0.0), (3.0, 0.05)])
    images, ranges = _truth(gpu, scene, cams)
    start = to_torch(scene, gpu)
    start[0] = start[0] * 1.05
    start[4] = start[4] + 0.3
    kept = [(c.rot.copy(), c.tran.copy()) for c in cams]

    def run(free):
        opt = TrainOptions(n_iters=100, n_iters_warmup=3, depth_weight=0.3 if rgbd else 0.0)
        tr = Trainer([t.clone() for t in start], list(cams), images, opt, max_pairs=1 << 20, depths=ranges if rgbd else None)
        assert tr._can_fuse_adam()
        if free:
            for i in range(3):
                tr.free_pose(i, 0.0, 0.0)
        with _Calls() as calls:
            vals = [tr.train_step(i, i % 3).clone() for i in range(12)]
        poses = [tr.pose(i) for i in range(3)]
        return (tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone(),
                tr.optimizer.accum_grad.clone(), torch.stack(vals)), calls.n, poses, tr

    (a, n_a, poses, tr), (b, n_b, _, _) = run(True), run(False)
    assert n_a == 12 and n_b == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], FlatGaussianParams([t.clone() for t in start]).flat_param)
    for i, (cam, (rot, tran)) in enumerate(zip(cams, poses)):
        assert rot.dtype == np.float64 and np.array_equal(rot, cam.rot.astype(np.float64))
        assert np.array_equal(tran, cam.tran.astype(np.float64))
        assert np.array_equal(cam.rot, kept[i][0]) and np.array_equal(cam.tran, kept[i][1])  # the caller's objects
        assert tr.cameras[i] is not cam and np.array_equal(tr.cameras[i].rot, cam.rot)  # replaced by copies
        assert all(fp.adam.k == 4 and not fp.pending for fp in tr._free.values())
    # the unfused step of a free view (fuse_adam off) is the same step too
    opt = TrainOptions(n_iters=100, n_iters_warmup=3, depth_weight=0.3 if rgbd else 0.0)
    tr_u = Trainer([t.clone() for t in start], list(cams), images, opt, max_pairs=1 << 20, depths=ranges if rgbd else None,
                   fuse_adam=False)
    for i in range(3):
        tr_u.free_pose(i, 0.0, 0.0)
    with _Calls() as calls:
        for i in range(12):
            tr_u.train_step(i, i % 3)
    assert calls.n == 0 and torch.equal(tr_u.flat.flat_param, a[0]) and torch.equal(tr_u.optimizer.exp_avg, a[1])


def test_trainer_free_pose_moves_only_its_view_and_refuses_view_parallelism(gpu):
    W, H = 160, 112
    scene = make_scene(3_000, W, H, seed=21)
    cams = _cams(W, H, [(-3.0, -0.15), (0.0, 0.0)])
    images, ranges = _truth(gpu, scene, cams)
    tr = Trainer([t.clone() for t in to_torch(scene, gpu)], list(cams), images, TrainOptions(n_iters_warmup=1, depth_weight=0.2),
                 depths=ranges)
    tr.free_pose(1, 1e-3, 1e-3)
    for i in range(6):
        tr.train_step(i, i % 2)
    assert tr._free[1].pending  # applied lazily: nobody has read the pose since the last step
    cam1 = tr.cameras[1]
    rot, tran = tr.pose(1)
    assert not tr._free[1].pending and tr.cameras[1] is not cam1
    assert np.array_equal(tr.cameras[1].rot, rot.astype(np.float32)) and np.array_equal(tr.cameras[1].tran, tran.astype(np.float32))
    assert not np.array_equal(rot, cams[1].rot.astype(np.float64)) and np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    assert tr.cameras[0] is cams[0] and np.array_equal(tr.pose(0)[0], cams[0].rot.astype(np.float64))
    tr.fix_pose(1)
    assert 1 not in tr._free and np.array_equal(tr.pose(1)[0], rot.astype(np.float32).astype(np.float64))
    with _Calls() as calls:
        tr.train_step(6, 1)
    assert calls.n == 0
    # view parallelism: a step on a free view raises before anything is rendered
    import torch.distributed as dist

    tr.free_pose(0, 1e-3, 1e-3)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29910 + os.getpid() % 80))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        tr.flat.force_collective = True
        assert tr.flat.collective_active()
        before = tr.flat.flat_param.clone()
        with pytest.raises(RuntimeError, match="free pose"):
            tr.train_step(7, 0)
        assert torch.equal(tr.flat.flat_param, before)
        tr.flat.force_collective = False
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------- e. joint refinement works
# Measured on an MI355X (profiles/pose_refine.txt): the end errors of the three freed views; asserted at 2 x these.
REFINE_RECORDED = [(2.812e-4, 1.387e-3), (1.496e-4, 8.762e-4), (2.383e-4, 1.241e-3)]  # (rotation, translation) of views 1 - 3 at the end
REFINE_LR = 5e-4        # TrackOptions' 2e-3 x 0.25, constant: 200 steps per view can travel 0.1, five times the perturbation
REFINE_STEPS = 800


def _perturbed(cam, seed):
    """test_pose_recovery's perturbation: 0.5 degrees about a random axis, 0.02 along a random direction."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    sh = rng.normal(size=3)
    c = copy.copy(cam)
    c.rot = (so3_exp_series(axis * math.radians(0.5)) @ cam.rot.astype(np.float64)).astype(np.float32)
    c.tran = (cam.tran.astype(np.float64) + sh / np.linalg.norm(sh) * 0.02).astype(np.float32)
    return c


def test_joint_refinement_recovers_perturbed_poses(gpu):
    """3,000 Gaussians, 160 x 112, four views with truth images and range maps; the map starts at the truth, view 0 is exact
    and fixed, views 1 - 3 start 0.5 degrees and 0.02 off and are free.  Every freed view ends closer to its true pose in
    rotation and in translation, view 0 is bit-unchanged, and the colour + depth training loss of the last round over the views
    is below that of the same run with the perturbed poses held fixed.

    Measured on an MI355X (profiles/pose_refine.txt): every freed view starts at (8.727e-03 rad, 2.000e-02) and ends at
    (2.812e-04, 1.387e-03), (1.496e-04, 8.762e-04), (2.383e-04, 1.241e-03); the loss of the last round is 0.004824 with the
    poses free against 0.062729 with the perturbed poses held fixed."""
    W, H = 160, 112
    scene = make_scene(3_000, W, H, seed=21)
    true_cams = _cams(W, H, [(0.0, 0.0), (-6.0, -0.3), (-3.0, -0.15), (3.0, 0.15)])
    images, ranges = _truth(gpu, scene, true_cams)
    start_cams = [true_cams[0]] + [_perturbed(c, 300 + i) for i, c in enumerate(true_cams[1:])]
    truth = [(c.rot.astype(np.float64), c.tran.astype(np.float64)) for c in true_cams]
    e0 = [pose_errors(c.rot, c.tran, *truth[i]) for i, c in enumerate(start_cams)]
    assert e0[0] == (0.0, 0.0) and all(abs(r - math.radians(0.5)) < 1e-4 and abs(t - 0.02) < 1e-4 for r, t in e0[1:])

    def run(free):
        opt = TrainOptions(n_iters=REFINE_STEPS + 1, n_iters_warmup=10, depth_weight=0.2)
        tr = Trainer([t.clone() for t in to_torch(scene, gpu)], list(start_cams), images, opt, max_pairs=1 << 20, depths=ranges)
        if free:
            for i in (1, 2, 3):
                tr.free_pose(i, REFINE_LR, REFINE_LR)
        tail = []
        for i in range(REFINE_STEPS):
            v = tr.train_step(i, i % 4)
            if i >= REFINE_STEPS - 4:
                tail.append((v[0] + tr.depth_loss.values[0]).clone())
        return tr, float(torch.stack(tail).sum())

    tr, loss_free = run(True)
    _, loss_fixed = run(False)
    e1 = [pose_errors(*tr.pose(i), *truth[i]) for i in range(4)]
    print("joint refinement, pose errors (rotation, translation) start -> end:")
    for i in range(4):
        print(f"  view {i}: ({e0[i][0]:.3e}, {e0[i][1]:.3e}) -> ({e1[i][0]:.3e}, {e1[i][1]:.3e})")
    print(f"  colour + depth loss of the last round over the four views: poses free {loss_free:.6f}, poses fixed {loss_fixed:.6f}")
    assert tr.cameras[0] is start_cams[0] and e1[0] == (0.0, 0.0)
    assert np.array_equal(tr.cameras[0].rot, true_cams[0].rot) and np.array_equal(tr.cameras[0].tran, true_cams[0].tran)
    for i in (1, 2, 3):
        assert e1[i][0] < e0[i][0] and e1[i][1] < e0[i][1], (i, e0[i], e1[i])
    assert loss_free < loss_fixed
    assert REFINE_RECORDED is not None, "no recorded end errors"
    for i in (1, 2, 3):
        assert e1[i][0] <= 2 * REFINE_RECORDED[i - 1][0] and e1[i][1] <= 2 * REFINE_RECORDED[i - 1][1], (i, e1[i])


# ------------------------------------------------------------------------------------------ f. Slam with refine_poses
W_, H_, N_FRAMES = 160, 120, 8
_SCENE, _RUN = {}, {}
# How far the worst keyframe pose of the refined run may lie above the unrefined run's (profiles/pose_refine.txt): a view's
# pose optimizer runs at a constant rate, so a pose that has arrived keeps moving by up to the rate per step and component;
# five rates (1e-3 rad, 1e-3 scene units) bound that wander generously and stay an order below one frame's motion (8.7e-3,
# 0.02).
SLAM_MARGIN_RATES = 5.0


def _scene(gpu):
    if not _SCENE:
        scene, cam = aux_case(20_000, W_, H_, seed=103)
        _SCENE["x"] = (to_torch(scene, gpu), cam, FrameRenderer(gpu, max_pairs=1 << 19, training=False, auto_grow=True,
                                                                occlusion_cull=False))
    return _SCENE["x"]


def _posed(cam, rot, tran):
    c = copy.copy(cam)
    c.rot, c.tran = np.asarray(rot, np.float32), np.asarray(tran, np.float32)
    return c


def _target(gpu, rot, tran):
    params, cam, r = _scene(gpu)
    img, _, d, a = r.forward(*params, _posed(cam, rot, tran), training=False, aux=True)
    rng = torch.where(a > 0.5, d / a.clamp_min(1e-3), torch.zeros_like(d))
    return img.contiguous().clone(), rng.contiguous().clone()


def _poses(cam, n):
    rng_ = np.random.default_rng(211)
    axis = rng_.normal(size=3)
    axis /= np.linalg.norm(axis)
    dR = so3_exp_series(axis * math.radians(0.5))
    u = rng_.normal(size=3)
    R, t = cam.rot.astype(np.float64), cam.tran.astype(np.float64)
    dt = u / np.linalg.norm(u) * 0.02 - (dR @ t - t)
    poses = [(R, t)]
    for _ in range(n - 1):
        R, t = poses[-1]
        poses.append((dR @ R, dR @ t + dt))
    return poses


def _frames(gpu):
    if "frames" not in _RUN:
        _, cam, _ = _scene(gpu)
        poses = _poses(cam, N_FRAMES)
        _RUN["frames"] = (poses, [_target(gpu, R, t) for R, t in poses])
    return _RUN["frames"]


def _slam_state(slam):
    tr = slam.trainer
    return ([tr.flat.flat_param.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone(),
             slam.keyframes.table.clone()],
            [(c.rot.copy(), c.tran.copy()) for c in tr.cameras], [(c.rot.copy(), c.tran.copy()) for c in slam.keyframes.cameras])


def _slam_run(gpu, refine):
    from gs_slam import Slam, SlamOptions, view_row

    _, cam, _ = _scene(gpu)
    poses, targets = _frames(gpu)
    slam = Slam(_posed(cam, *poses[0]), SlamOptions(overlap_min=0.0, keyframe_every=3, refine_poses=refine), gpu)
    rows = []
    for f, ((R, t), (img, rng)) in enumerate(zip(poses, targets)):
        before = _slam_state(slam) if slam.trainer is not None else None
        flat = slam.trainer.flat if slam.trainer is not None else None
        frame = slam.step(img, rng)
        unchanged = None
        if before is not None:
            after = _slam_state(slam)
            unchanged = (slam.trainer.flat is flat and all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
                         and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                                 for x, y in ((before[1], after[1]), (before[2], after[2])) for a, b in zip(x, y)))
        # after every frame: table row == view_row(keyframe camera), and the trainer's camera agrees
        for i, kc in enumerate(slam.keyframes.cameras):
            assert np.array_equal(slam.keyframes.table[i].cpu().numpy(), view_row(kc)), (f, i)
            tc = slam.trainer.cameras[i]
            assert np.array_equal(tc.rot, kc.rot) and np.array_equal(tc.tran, kc.tran), (f, i)
        assert not slam.trainer._free
        rows.append(dict(frame=frame, err=pose_errors(frame.rot, frame.tran, R, t), unchanged=unchanged,
                         last=(slam.tracker._history[-1] if slam.tracker._history else None)))
    kf_frames = [f for f, row in enumerate(rows) if row["frame"].keyframe]
    kf_err = [pose_errors(c.rot, c.tran, *poses[f]) for f, c in zip(kf_frames, slam.keyframes.cameras)]
    return dict(slam=slam, rows=rows, kf_frames=kf_frames, kf_err=kf_err)


def test_slam_refines_the_window_poses(gpu):
    from gs_slam import SlamOptions, view_row

    _, cam, _ = _scene(gpu)
    poses, _t = _frames(gpu)
    off, on = _slam_run(gpu, False), _slam_run(gpu, True)
    o = on["slam"].opt
    assert on["kf_frames"] == off["kf_frames"] == [0, 3, 6]
    print("slam with refine_poses, keyframe pose errors (rotation, translation), unrefined -> refined:")
    for k, f in enumerate(on["kf_frames"]):
        print(f"  keyframe {k} (frame {f}): ({off['kf_err'][k][0]:.3e}, {off['kf_err'][k][1]:.3e}) -> "
              f"({on['kf_err'][k][0]:.3e}, {on['kf_err'][k][1]:.3e})")
    print("  per frame (as reported by the frame), unrefined -> refined: " + ", ".join(
        f"{f}: ({a['err'][0]:.2e}, {a['err'][1]:.2e}) -> ({b['err'][0]:.2e}, {b['err'][1]:.2e})"
        for f, (a, b) in enumerate(zip(off["rows"], on["rows"]))))
    # the default leaves the loop alone: no frame of the unrefined run carries refined poses
    assert all(row["frame"].refined == {} for row in off["rows"])
    # keyframe 0 is the gauge: pose and table row bit-unchanged
    first = _posed(cam, *poses[0])
    kc0 = on["slam"].keyframes.cameras[0]
    assert np.array_equal(kc0.rot, first.rot) and np.array_equal(kc0.tran, first.tran)
    assert np.array_equal(on["slam"].keyframes.table[0].cpu().numpy(), view_row(first))
    moved = 0
    for f, row in enumerate(on["rows"]):
        fr = row["frame"]
        if not fr.keyframe:  # map, optimizer state, poses and table untouched, bit for bit
            assert row["unchanged"] is True and fr.refined == {}, f
            continue
        assert set(fr.refined) <= set(fr.window) - {0}, (f, fr.window, sorted(fr.refined))
        if f == 0:
            assert fr.refined == {}
            continue
        assert set(fr.refined) == set(fr.window) - {0}, (f, fr.window, sorted(fr.refined))  # every freed view took steps
        moved += len(fr.refined)
        new = fr.window[0]
        assert np.array_equal(fr.rot, fr.refined[new][0]) and np.array_equal(fr.tran, fr.refined[new][1])
        assert fr.rot.dtype == np.float64 and not np.array_equal(fr.rot, fr.tracked.rot)
        assert np.abs(fr.rot @ fr.rot.T - np.eye(3)).max() < 1e-6  # (a float32 start, float64 steps)
        # the tracker's motion history starts from the refined pose
        assert np.array_equal(row["last"][0], fr.rot) and np.array_equal(row["last"][1], fr.tran)
    assert moved >= 3
    margin = SLAM_MARGIN_RATES * np.array([o.pose_lr_rot, o.pose_lr_tran])
    worst_off, worst_on = np.max(np.array(off["kf_err"]), axis=0), np.max(np.array(on["kf_err"]), axis=0)
    print(f"  worst keyframe error: unrefined ({worst_off[0]:.3e}, {worst_off[1]:.3e}), refined ({worst_on[0]:.3e}, "
          f"{worst_on[1]:.3e}), margin ({margin[0]:.1e}, {margin[1]:.1e})")
    assert np.all(worst_on <= worst_off + margin), (worst_on, worst_off, margin)


def test_keyframe_set_set_pose(gpu):
    from gs_slam import KeyframeSet, view_row

    cam = make_camera(160, 120, yaw_deg=2.0)
    ks = KeyframeSet(capacity=4, device=gpu)
    img, rng = torch.zeros(120, 160, 3, device=gpu), torch.ones(120, 160, device=gpu)
    ks.add(cam, img, rng)
    ks.add(make_camera(160, 120, yaw_deg=4.0), img, rng)
    table = ks.table.clone()
    rot = so3_exp_series(np.array([0.01, -0.02, 0.005])) @ cam.rot.astype(np.float64)
    old = ks.cameras[1]
    ks.set_pose(1, rot, [0.1, 0.2, 0.3])
    assert ks.cameras[1] is not old and np.array_equal(ks.cameras[1].rot, rot.astype(np.float32))
    assert np.array_equal(ks.table[1].cpu().numpy(), view_row(ks.cameras[1]))
    assert torch.equal(ks.table[0], table[0]) and torch.equal(ks.table[2:], table[2:]) and not torch.equal(ks.table[1], table[1])
    with pytest.raises(IndexError):
        ks.set_pose(2, rot, [0, 0, 0])
    assert torch.equal(ks.table[0], table[0])
