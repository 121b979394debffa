"""GPU tier of the depth alignment (csrc/icp.hip through the C ABI, gs_icp.IcpAligner) against tests/icp_ref.py: the model
maps bit for bit, one step's counts exactly and its sums within the fp32 summation bound, the solve and the state update, the
refusing statuses, repeatability over the workspace's contents, and the whole alignment on the analytic room corner."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import icp_ref as R
from track_ref import perturbed_start, pose_errors

pytestmark = pytest.mark.gpu

DIST_MAX, COS_MIN, DAMPING = 0.2, 0.0, 1e-6
_CACHE = {}


def _pp(cam):
    from gaussian import _lib

    c = _lib.GsSeedCameraPP()
    c.cam.rot = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    c.cam.focal_x, c.cam.focal_y = cam.focal_x, cam.focal_y
    c.cam.width, c.cam.height = cam.width, cam.height
    c.pp_dx, c.pp_dy = cam.dx, cam.dy
    return c


def _dev(a, gpu, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(gpu)


def _model_maps(gpu, cam, depth, alpha, step=1, alpha_min=R.ALPHA_MIN, edge_rel=R.EDGE_REL):
    from gaussian import _lib

    d = _dev(depth, gpu)
    a = _dev(alpha, gpu) if alpha is not None else None
    # (filled with a pattern: every pixel of both maps must be written)
    vertex = torch.full((cam.height, cam.width, 4), 7.0, dtype=torch.float32, device=gpu)
    normal = torch.full((cam.height, cam.width, 4), 7.0, dtype=torch.float32, device=gpu)
    assert vertex.numel() * 4 == _lib.gs_icp_model_bytes(cam.height, cam.width)
    c, o = _pp(cam), _lib.GsIcpModelOpts(alpha_min, edge_rel, step)
    _lib.check(_lib.gs_icp_model_maps(d.data_ptr(), a.data_ptr() if a is not None else None, C.byref(c), C.byref(o),
                                      vertex.data_ptr(), normal.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "gs_icp_model_maps")
    return vertex, normal


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ 1. model maps
@pytest.mark.parametrize("pp", [(0.0, 0.0), R.PP_OFFSET], ids=["centred", "pp"])
@pytest.mark.parametrize("size", R.MAP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_maps_match_the_float32_restatement_bit_for_bit(gpu, size, pp):
    """Vertices, normals and both flags, from (D, A) with A straddling alpha_min and from a plain range map, normal_step 1 and
    2; the range map has holes and a depth step, so the edge rule and the border both decide."""
    H, W = size
    cam, D, A, rho = R.maps_case(H, W, H + W, pp)
    for step in (1, 2):
        for depth, alpha in ((D, A), (rho, None)):
            vertex, normal = _model_maps(gpu, cam, depth, alpha, step)
            Vr, Nr = R.model_maps(depth, alpha, cam, R.ALPHA_MIN, R.EDGE_REL, step)
            assert np.array_equal(_bits(vertex), _bits(Vr)), (size, pp, step, alpha is None)
            assert np.array_equal(_bits(normal), _bits(Nr)), (size, pp, step, alpha is None)
            assert 0 < Nr[..., 3].sum() < Vr[..., 3].sum() < H * W  # (holes, edges and the border all took something)
    # the edge rule decides: without it more normals are valid, and the centred ray is the offset ray at (0, 0) by construction
    _, n_off = _model_maps(gpu, cam, rho, None, 1, edge_rel=-1.0)
    assert np.array_equal(_bits(n_off), _bits(R.model_maps(rho, None, cam, R.ALPHA_MIN, -1.0, 1)[1]))
    assert n_off[..., 3].sum().item() > R.model_maps(rho, None, cam)[1][..., 3].sum()


# ------------------------------------------------------------------------------------------------------------ 2. a step
class _Step:
    """State, log and workspace of gs_icp_step calls on one frame size."""

    def __init__(self, gpu, cam, mcam, z, vertex, normal, rows=4, fill=None):
        from gaussian import _lib

        self.lib, self.gpu = _lib, gpu
        self.cam, self.mcam, self.z, self.vertex, self.normal = _pp(cam), _pp(mcam), _dev(z, gpu), vertex, normal
        self.rows = rows
        self.state = torch.zeros(16, dtype=torch.float64, device=gpu)
        self.log = torch.full((rows, 40), -1.0, dtype=torch.float64, device=gpu)
        assert self.log.numel() * 8 == _lib.gs_icp_log_bytes(rows)
        self.size = (cam.height, cam.width)
        self.fill = fill

    def reset(self, Rm, t):
        Rm, t = np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
        self.lib.check(self.lib.gs_icp_reset(self.state.data_ptr(), self.log.data_ptr(), self.rows, (C.c_double * 9)(*Rm),
                                             (C.c_double * 3)(*t), torch.cuda.current_stream().cuda_stream), "gs_icp_reset")

    def step(self, row, stride, dist_max=DIST_MAX, cos_min=COS_MIN, damping=DAMPING, min_count=6):
        ws = torch.empty(int(self.lib.gs_icp_workspace_bytes(*self.size, stride)), dtype=torch.uint8, device=self.gpu)
        if self.fill is not None:
            ws.fill_(self.fill)
        o = self.lib.GsIcpOpts(stride, dist_max, cos_min, min_count, damping)
        self.lib.check(self.lib.gs_icp_step(self.z.data_ptr(), C.byref(self.cam), self.vertex.data_ptr(), self.normal.data_ptr(),
                                            C.byref(self.mcam), C.byref(o), self.state.data_ptr(), self.log.data_ptr(), self.rows,
                                            row, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                       "gs_icp_step")

    def read(self):
        s = self.state.cpu().numpy()
        it = int(s[12:13].view(np.int32)[0])
        return s[0:9].reshape(3, 3).copy(), s[9:12].copy(), it, self.log.cpu().numpy()


STEP_CASES = [(7, 9), (48, 64), (120, 160), (187, 250)]


def _check_step(gpu, k, strides, big_from=4000):
    Vr, Nr = R.model_maps(k["zm"], None, k["mcam"])
    vertex, normal = _model_maps(gpu, k["mcam"], k["zm"], None)
    assert np.array_equal(_bits(vertex), _bits(Vr)) and np.array_equal(_bits(normal), _bits(Nr))
    run = _Step(gpu, k["cam"], k["mcam"], k["z"], vertex, normal, rows=len(strides), fill=0xFF)
    for row, stride in enumerate(strides):
        run.reset(k["R"], k["t"])  # (also zeroes the log: one row per reset is compared)
        run.step(row, stride)
        Rn, tn, it, log = run.read()
        terms, kept, meas = R.step_terms(k["z"], k["cam"], Vr, Nr, k["mcam"], k["R"], k["t"], stride, DIST_MAX, COS_MIN)
        got = log[row]
        # exact counts
        assert (int(got[0]), int(got[1])) == (kept, meas), (stride, got[:2], kept, meas)
        ys, xs = R.lattice(k["cam"].height, k["cam"].width, stride)
        if len(ys) * len(xs) >= big_from:
            assert kept >= 1000, (stride, kept)
        # the 28 sums against a float64 sum of the restatement's fp32 terms: m = the terms one thread adds sequentially = the
        # chunks of 256 lattice pixels in a workgroup's run (1 up to 262,144 lattice pixels: the grid cap of 1,024 workgroups);
        # the butterfly adds 6 levels and the four waves 3 more -- the "+ 10" covers them
        m = math.ceil(math.ceil(len(ys) * len(xs) / 256) / 1024) if len(ys) * len(xs) else 1
        t64 = terms.astype(np.float64)
        ref, mag = t64.sum(axis=0), np.abs(t64).sum(axis=0)
        sums = np.concatenate([got[3:30], got[2:3]])
        bound = (m + 10) * 2.0 ** -24 * mag
        assert np.all(np.abs(sums - ref) <= bound), (stride, m, np.abs(sums - ref) / np.maximum(bound, 1e-300))
        assert it == 1 and int(got[38]) == stride and got[39] == 0.0
        # the solve, from the log's own A and b
        A, b, _ = R.unpack(sums)
        x, lam = got[30:36], got[37]
        if kept >= 6:  # (min_count = 6; the damped matrix of every case here is positive definite)
            assert got[36] == 0.0
            assert abs(lam - DAMPING * np.trace(A) / 6.0) <= 1e-15 * abs(lam) + 1e-300
            res = (A + lam * np.eye(6)) @ x + b
            assert np.linalg.norm(res) <= 1e-10 * (np.linalg.norm(A) * np.linalg.norm(x) + np.linalg.norm(b)), (stride, res)
            Rw, tw = R.update(k["R"], k["t"], x)
            assert np.abs(Rn - Rw).max() <= 1e-12 and np.abs(tn - tw).max() <= 1e-12
        else:
            assert got[36] == 1.0 and np.all(x == 0)
            assert np.array_equal(Rn, np.asarray(k["R"], np.float64)) and np.array_equal(tn, np.asarray(k["t"], np.float64))
        m_seen = _CACHE.setdefault("m_seen", set())
        m_seen.add(m)


@pytest.mark.parametrize("size", STEP_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_step_counts_exactly_and_sums_within_the_fp32_bound(gpu, size):
    """Strides 1, 2 and 4 at a state 1 degree / 0.03 off the identity, the frame 2 degrees / 0.08 off the model view."""
    H, W = size
    _check_step(gpu, R.step_case(H, W, H + W), (1, 2, 4))


def test_one_step_beyond_the_grid_cap(gpu):
    """640 x 480 at stride 1: 307,200 lattice pixels are 1,200 chunks -- beyond the cap of 1,024 workgroups, so every workgroup
    adds a run of two chunks (m = 2) -- and 600 partial rows, more than the finalize workgroup has threads."""
    _check_step(gpu, R.step_case(480, 640, 1120), (1,))
    assert 2 in _CACHE["m_seen"]


def test_one_step_between_differing_cameras(gpu):
    """A 160 x 120 frame with its own principal-point offset against a 250 x 187 model map with the offset (7.3, -4.6)."""
    _check_step(gpu, R.step_case(120, 160, 5, model_size=(187, 250), model_pp=R.PP_OFFSET, frame_pp=(-2.5, 3.25)), (1, 2, 4))


# ---------------------------------------------------------------------------------------------------------- 3. the solve
def test_too_few_pixels_and_an_invalid_model_leave_the_state_alone(gpu):
    k = R.step_case(48, 64, 112)
    vertex, normal = _model_maps(gpu, k["mcam"], k["zm"], None)
    run = _Step(gpu, k["cam"], k["mcam"], k["z"], vertex, normal, rows=4)
    run.reset(k["R"], k["t"])
    kept = R.step_terms(k["z"], k["cam"], *R.model_maps(k["zm"], None, k["mcam"]), k["mcam"], k["R"], k["t"], 2, DIST_MAX,
                        COS_MIN)[1]
    run.step(0, 2, min_count=kept + 1)   # one pixel short
    run.step(1, 2, min_count=kept)       # exactly enough: this one moves
    Rn, tn, it, log = run.read()
    assert log[0, 36] == 1.0 and log[0, 0] == kept and np.all(log[0, 30:36] == 0)
    assert log[1, 36] == 0.0 and np.any(log[1, 30:36] != 0) and it == 2
    assert not np.array_equal(Rn, k["R"])
    # an all-invalid model: nothing is kept, whatever the frame holds
    empty = torch.zeros_like(normal)
    for min_count, status in ((6, 1.0), (0, 2.0)):  # too few; with no minimum the zero matrix has no positive pivot
        run = _Step(gpu, k["cam"], k["mcam"], k["z"], vertex, empty, rows=2)
        run.reset(k["R"], k["t"])
        before = run.state.clone()
        run.step(0, 1, min_count=min_count)
        after = run.state.clone()
        _, _, it, log = run.read()
        assert log[0, 36] == status and log[0, 0] == 0 and log[0, 1] > 0 and np.all(log[0, 2:36] == 0)
        assert torch.equal(before[:12].view(torch.int64), after[:12].view(torch.int64)) and it == 1  # bitwise unchanged
    # a frame with no measurement at all
    run = _Step(gpu, k["cam"], k["mcam"], np.zeros_like(k["z"]), vertex, normal, rows=1)
    run.reset(k["R"], k["t"])
    run.step(0, 1)
    assert run.read()[3][0, 36] == 1.0 and run.read()[3][0, 1] == 0


# ------------------------------------------------------------------------------------- 4. and 5. the aligner on the corner
def _aligner(gpu, **kw):
    from gs_icp import IcpAligner, IcpOptions

    cam = R.corner_camera()

    class Camera:  # what gs_seed.seed_camera reads
        rot, tran = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        focal_x = focal_y = cam.focal_x
        width, height = cam.width, cam.height

    return IcpAligner(Camera(), IcpOptions(**kw), gpu)


def _corner_align(gpu, aligner, rot_true, angle, shift, init_given=False):
    z = _dev(R.corner_range(rot_true, R.CORNER_TRAN), gpu)
    rot0, tran0 = perturbed_start(rot_true, R.CORNER_TRAN, angle_deg=angle, shift=shift)
    aligner.set_model(_dev(R.corner_range(rot0, tran0), gpu), None, rot0, tran0)
    res = aligner.align(z, (rot0, tran0) if init_given else None)
    return pose_errors(rot0, tran0, rot_true, R.CORNER_TRAN), pose_errors(res.rot, res.tran, rot_true, R.CORNER_TRAN), res


def test_align_is_repeatable_whatever_the_workspace_held(gpu):
    from gaussian import _lib

    runs = []
    for fill in (0xFF, 0x00):
        a = _aligner(gpu)
        for stride, _ in R.STAGES:
            a._workspace(a._cam, stride).fill_(fill)
        a._dev.fill_(float("nan") if fill else 0.0)
        _, _, res = _corner_align(gpu, a, R.CORNER_ROT, 2.0, 0.08)
        runs.append((a._dev.cpu().numpy().copy(), res))
    (d0, r0), (d1, r1) = runs
    # the state (13 of the 16 doubles in front of the log: the rest is padding nobody writes) and the log
    assert np.array_equal(d0[:13].view(np.uint64), d1[:13].view(np.uint64))
    assert np.array_equal(d0[16:].view(np.uint64), d1[16:].view(np.uint64))
    assert np.array_equal(r0.rot.view(np.uint64), r1.rot.view(np.uint64)) and np.array_equal(r0.tran.view(np.uint64),
                                                                                             r1.tran.view(np.uint64))
    assert np.array_equal(r0.log.view(np.uint64), r1.log.view(np.uint64)) and r0.accepted and r1.accepted
    assert r0.log.shape == (19, _lib.GS_ICP_LOG_DOUBLES) and [int(s) for s in r0.log[:, 38]] == [4] * 4 + [2] * 5 + [1] * 10


@pytest.mark.parametrize("angle,shift", R.STARTS)
def test_align_converges_on_the_corner_with_one_host_read(gpu, angle, shift, monkeypatch):
    """The starts of the CPU tier, the model given as the corner's exact range map from the start pose: at most a tenth of
    both start errors, accepted, and exactly one synchronising copy for the whole alignment."""
    import gs_icp

    reads = []
    real = gs_icp._read
    monkeypatch.setattr(gs_icp, "_read", lambda host, dev: (reads.append(dev.numel()), real(host, dev))[1])
    a = _aligner(gpu)
    start, end, res = _corner_align(gpu, a, R.CORNER_ROT, angle, shift)
    print(f"start {start} -> end {end}; accepted {res.accepted}, rmse {res.rmse:.3e}, inliers {res.inliers} / {res.measured}")
    assert reads == [16 + 19 * 40]
    assert res.accepted and res.iterations == 19
    assert end[0] <= 0.1 * start[0] and end[1] <= 0.1 * start[1], (start, end)
    # the same alignment with the start given as `init` against a model rendered elsewhere: the model at the TRUE pose, the
    # frame believed at the start pose -- the relative motion then starts off the identity and ends at it
    z = _dev(R.corner_range(R.CORNER_ROT, R.CORNER_TRAN), gpu)
    rot0, tran0 = perturbed_start(R.CORNER_ROT, R.CORNER_TRAN, angle_deg=angle, shift=shift)
    a.set_model(z, None, R.CORNER_ROT, R.CORNER_TRAN)
    res2 = a.align(z, (rot0, tran0))
    end2 = pose_errors(res2.rot, res2.tran, R.CORNER_ROT, R.CORNER_TRAN)
    assert res2.accepted and end2[0] <= 0.1 * start[0] and end2[1] <= 0.1 * start[1], (start, end2)
    assert len(reads) == 2
    # the first iteration starts at the identity exactly: its counts are the float32 restatement's
    cam = R.corner_camera()
    V, N = R.model_maps(R.corner_range(rot0, tran0).astype(np.float32), None, cam)
    _, kept, meas = R.step_terms(R.corner_range(R.CORNER_ROT, R.CORNER_TRAN).astype(np.float32), cam, V, N, cam, np.eye(3),
                                 np.zeros(3), 4, 0.2, 0.0)
    assert (int(res.log[0, 0]), int(res.log[0, 1])) == (kept, meas)


def test_a_declined_alignment_returns_the_init_pose(gpu):
    a = _aligner(gpu, min_inlier_share=1.0)  # nothing reaches an inlier share of one: the corner's edges have no normals
    rot0, tran0 = perturbed_start(R.CORNER_ROT, R.CORNER_TRAN, angle_deg=2.0, shift=0.08)
    start, end, res = _corner_align(gpu, a, R.CORNER_ROT, 2.0, 0.08)
    assert not res.accepted and np.array_equal(res.rot, rot0) and np.array_equal(res.tran, tran0)
    assert res.inliers < res.measured and np.all(res.log[:, 36] == 0)


@pytest.mark.parametrize("angle,shift", R.STARTS)
def test_the_sliding_corner_on_the_device(gpu, angle, shift):
    """The corner without its third plane: printed, and only the residual is asserted to fall -- the guard cannot see a slide."""
    start, end, res = _corner_align(gpu, _aligner(gpu), R.SLIDING_ROT, angle, shift)
    rmse = np.sqrt(res.log[:, 2] / np.maximum(res.log[:, 0], 1))
    print(f"sliding corner from {start}: accepted {res.accepted}, end {end}, rmse {rmse[0]:.3e} -> {rmse[-1]:.3e}, "
          f"inliers {res.inliers} / {res.measured}")
    assert rmse[-1] < rmse[0]
