"""CPU tier of the depth / alpha maps (GS_FRAME_AUX, include/gs_abi.h): the aux workspace size query, the validation of a
flagged frame, the refusal of the fused-Adam backward, and the register / scratch budgets of the aux kernels read from the
built code objects.  No kernel is launched here."""
import ctypes as C
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2


from gs_testutil import fake_frame as _frame  # (plain unless aux=True)


def test_aux_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_frame_aux_workspace_bytes
    assert _lib.GS_FRAME_AUX == 2048
    for tr in (0, 1):
        assert q(1000, 64, 48, tr) > 0
        assert q(1000, 64, 48, tr) % 256 == 0
        assert q(2_000_000, 64, 48, tr) >= q(1000, 64, 48, tr)       # monotone in the pair capacity
        assert q(1000, 1920, 1080, tr) >= q(1000, 64, 48, tr)        # ... and in the image size
    assert q(2_000_000, 64, 48, 1) > q(1000, 64, 48, 1)
    assert q(1000, 1920, 1080, 1) > q(1000, 64, 48, 1)
    assert q(100_000, 640, 480, 1) > q(100_000, 640, 480, 0)         # the checkpoints are kept by training frames only
    # the (D, A) checkpoints: 8 bytes x 256 pixels per bucket of the capacity
    T = (640 // 16) * (480 // 16)
    assert q(100_000, 640, 480, 1) >= 8 * 256 * (100_000 // 64 + T + 1)
    for bad in ((-1, 64, 48, 1), (1000, 0, 48, 1), (1000, 64, 0, 0), (1000, -5, 48, 0)):
        assert q(*bad) == 0
    # the main workspace does not depend on the flag (its size query has no aux argument at all)
    assert _lib.gs_frame_workspace_bytes(1000, 50_000, 128, 96, 3, 1) > 0


def test_flagged_frame_validation_is_host_only():
    from gaussian import _lib

    # gs_frame_binning_variant validates the description and answers on the host (negative: does not validate)
    assert _lib.gs_frame_binning_variant(C.byref(_frame())) >= 0
    assert _lib.gs_frame_binning_variant(C.byref(_frame(aux=True))) >= 0
    assert _lib.gs_frame_binning_variant(C.byref(_frame(aux=True, training=0))) >= 0
    f = _frame(aux=True)
    f.aux_workspace = None
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    assert b"aux" in _lib.gs_last_error()
    f = _frame(aux=True)
    f.aux_workspace_bytes -= 256
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    assert b"aux workspace too small" in _lib.gs_last_error()
    f = _frame(aux=True)
    f.aux_workspace += 16  # not 256-byte aligned
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    f = _frame(aux=True)
    f.aux_padded = None  # a training frame's backward reads the raw sums
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    f = _frame(aux=True, training=0)
    f.aux_padded = None  # ... an inference frame needs none
    assert _lib.gs_frame_binning_variant(C.byref(f)) >= 0
    # an all-zero descriptor with the flag: rejected, nothing launched
    z = _lib.GsFrame()
    z.flags = _lib.GS_FRAME_AUX
    assert _lib.gs_frame_forward(C.byref(z), None) == GS_E_INVALID
    assert _lib.gs_frame_backward(C.byref(z), None, None, None, None, None, None, None) == GS_E_INVALID


def test_fused_adam_backward_refuses_aux_frames():
    from gaussian import _lib

    adam = _lib.GsAdamFused()
    rc = _lib.gs_frame_backward_adam(C.byref(_frame(aux=True)), 1 << 41, C.byref(adam), None)
    assert rc == GS_E_UNSUPPORTED
    assert b"GS_FRAME_AUX" in _lib.gs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Register / scratch budgets of the aux kernels (the read-out of tests/test_kernel_resources.py).  Limits proposed from the
# built code objects: rgb forward 140 / 142 VGPRs (three waves per SIMD: the four accumulators and the staged depth do not
# fit the plain kernel's 128), degree 2 at its plain kernel's 168 with a few spills outside the loop, degree 3 at 256
# without scratch; backward rgb 116 (four waves), degree 2 168 (three waves, a few spills outside the per-Gaussian loop) and
# degree 3 255 (two waves: one step below the plain kernels, whose budgets spilled inside the loop here);
# the per-Gaussian depth sums 26 VGPRs.
AUX_BUDGETS = [
    (("raster_aux_forward_kernelILi3ELb0E",), 168, False),
    (("raster_aux_forward_kernelILi3ELb1E",), 168, False),
    (("raster_aux_forward_kernelILi27ELb0E",), 168, True),
    (("raster_aux_forward_kernelILi27ELb1E",), 168, True),
    (("raster_aux_forward_kernelILi48ELb0E",), 256, True),
    (("raster_aux_forward_kernelILi48ELb1E",), 256, True),
    (("raster_aux_backward_kernelILi3E",), 128, False),
    (("raster_aux_backward_kernelILi27E",), 168, True),
    (("raster_aux_backward_kernelILi48E",), 256, True),
    (("frame_aux_depth_backward_kernelILi3E",), 64, False),
    (("frame_aux_depth_backward_kernelILi27E",), 64, False),
    (("frame_aux_depth_backward_kernelILi48E",), 64, False),
]
AUX_HOT_LOOPS = [
    (("raster_aux_forward_kernelILi3ELb0E",), "v_exp_f32", 8),
    (("raster_aux_forward_kernelILi3ELb1E",), "v_exp_f32", 8),
    (("raster_aux_forward_kernelILi27ELb0E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi27ELb1E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi48ELb0E",), "v_exp_f32", 32),
    (("raster_aux_forward_kernelILi48ELb1E",), "v_exp_f32", 32),
    (("raster_aux_backward_kernelILi3E",), "v_exp_f32", 4),
    (("raster_aux_backward_kernelILi27E",), "v_exp_f32", 4),
    (("raster_aux_backward_kernelILi48E",), "v_exp_f32", 4),
]


@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


def _pick(d, parts):
    hits = [k for k in d if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, hits)
    return hits[0]


@pytest.mark.parametrize("parts,vgprs,scratch_ok", AUX_BUDGETS, ids=[b[0][0] for b in AUX_BUDGETS])
def test_aux_kernel_fits_its_register_budget(kernels, parts, vgprs, scratch_ok):
    k = kernels[_pick(kernels, parts)]
    assert k[".vgpr_count"] <= vgprs, (k[".name"], k[".vgpr_count"])
    if not scratch_ok:
        assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, k[".name"]


def test_aux_kernels_keep_their_lds_budgets(kernels):
    # rgb forward: 16 one-wave workgroups per CU fit the LDS; rgb backward: four waves per SIMD
    assert kernels[_pick(kernels, ("raster_aux_forward_kernelILi3ELb0E",))][".group_segment_fixed_size"] * 16 <= 160 * 1024
    assert kernels[_pick(kernels, ("raster_aux_backward_kernelILi3E",))][".group_segment_fixed_size"] * 16 <= 160 * 1024


@pytest.fixture(scope="module")
def disassembly():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_loops
    from test_kernel_resources import LIB

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    if not (os.path.exists(isa_loops.OBJDUMP) or shutil.which(isa_loops.OBJDUMP)):
        pytest.skip("llvm-objdump not found")
    return isa_loops, isa_loops.disassemble_library()


@pytest.mark.parametrize("parts,marker,at_least", AUX_HOT_LOOPS, ids=[h[0][0] for h in AUX_HOT_LOOPS])
def test_aux_hot_loop_is_free_of_scratch_instructions(disassembly, parts, marker, at_least):
    isa, dis = disassembly
    insns = dis[_pick(dis, parts)]
    cands = [(lo, hi) for lo, hi in isa.loops(insns) if isa.count(insns, lo, hi, marker) >= at_least]
    assert cands, (parts, "no loop with", at_least, marker)
    inner = [(lo, hi) for lo, hi in cands if not any((l2, h2) != (lo, hi) and lo <= l2 and h2 <= hi for l2, h2 in cands)]
    for lo, hi in inner:
        assert isa.count(insns, lo, hi, "scratch_") == 0, (parts, lo, hi)


# ---------------------------------------------------------------------------------------------------------------------
# The yardstick of the aux gradient tests (tests/gs_testutil.py: OracleFrame.aux_maps / aux_backward / aux_backward_f64),
# checked before it judges a kernel.
PAR_NAMES = ("pos", "quat", "scale", "opa", "rgb")


def _small_case(shift, use_sh=False):
    import numpy as np

    from gs_testutil import OracleFrame, aux_case

    scene, cam = aux_case(1500, 64, 48, seed=13, use_sh=use_sh)
    scene.opa += np.float32(shift)
    return OracleFrame(scene, cam)


def test_backward_f64_is_unchanged_by_its_split():
    """OracleFrame.backward_f64 = _rows_f64 + _chain_f64 returns, bit for bit, what the undivided method returned: the
    fixture holds its rows and parameter gradients as recorded before the split (700 Gaussians at 64 x 48, the aux tests'
    camera, white-noise dL/dimage of seed 41 through robust_grad_image)."""
    import numpy as np

    from gs_testutil import OracleFrame, aux_case

    gold = np.load(os.path.join(ROOT, "tests", "golden", "backward_f64_split.npz"))
    scene, cam = aux_case(700, 64, 48, seed=3)
    of = OracleFrame(scene, cam)
    gimg, _ = of.robust_grad_image(np.random.default_rng(41).normal(size=of.image.shape).astype(np.float32))
    rows, par = of.backward_f64(gimg)
    assert len(of.ids) == len(gold["rows_opa"]) > 1000
    for name, got in zip(("pos", "rgb", "opa", "cov"), rows):
        assert got.dtype == np.float64 and np.array_equal(got, gold["rows_" + name]), name
    for name in PAR_NAMES:
        assert par[name].dtype == np.float64 and np.array_equal(par[name], gold["param_" + name]), name
        assert np.abs(par[name]).max() > 0


@pytest.mark.parametrize("shift,use_sh", [(0.0, False), (-4.0, False), (-4.0, True)],
                         ids=["saturated", "translucent", "translucent-sh"])
def test_aux_oracle_fp32_against_fp64(shift, use_sh):
    """aux_backward (fp32 terms) against aux_backward_f64 on a saturated and a translucent scene, all three gradients and
    the maps alone: (1) within the tolerance the kernels are held to against it (assert_grads_close, defaults) -- measured
    at most 0.08 of it --; (2) the maps' relative error against the double evaluation is, quantile by quantile, within
    CALIB_K (CALIB_K_MAX at the maximum) of what the same fp32 arithmetic has on the IMAGE's gradient of the same scene
    (measured 0.5 ... 2.2 x): posing the maps as colours does not make the yardstick any less accurate than the one the
    image tests use."""
    import numpy as np

    from gs_testutil import (CALIB_K, CALIB_K_MAX, CALIB_QS, assert_grads_close, rel_error_quantiles, robust_aux_grads,
                             saturated_share)

    of = _small_case(shift, use_sh)
    sat = saturated_share(of)
    assert (sat > 0.9) if shift == 0.0 else (sat < 0.01), sat
    gimg, gd, ga, n_masked = robust_aux_grads(of, 17)
    assert n_masked < 0.005 * of.image.shape[0] * of.image.shape[1]
    ref_i, _ = of.backward(gimg, with_scale=True)
    _, truth_i = of.backward_f64(gimg)
    for what, gi in (("all", gimg), ("maps", None)):
        ref, scale = of.aux_backward(gi, gd, ga)
        truth = of.aux_backward_f64(gi, gd, ga)
        assert_grads_close([ref[k] for k in PAR_NAMES], truth, scale, f"oracle fp32 vs fp64, {what}")
        if gi is None:
            assert np.all(ref["rgb"] == 0) and np.all(truth["rgb"] == 0)
            for k in ("pos", "quat", "scale", "opa"):
                qa, qi = rel_error_quantiles(ref[k], truth[k]), rel_error_quantiles(ref_i[k], truth_i[k])
                print(f"aux oracle shift {shift} {k}: maps", ["%.1e" % v for v in qa], "image", ["%.1e" % v for v in qi])
                for a, b, q in zip(qa, qi, CALIB_QS):
                    assert a <= (CALIB_K_MAX if q == 1.0 else CALIB_K) * b, (k, q, a, b)
    # the terms add up: the image alone + the maps alone = all three (linear; fp64 sums of the same rows)
    t_all, t_maps = of.aux_backward_f64(gimg, gd, ga), of.aux_backward_f64(None, gd, ga)
    t_d, t_a = of.aux_backward_f64(None, gd, None), of.aux_backward_f64(None, None, ga)
    for k in PAR_NAMES:
        s = np.abs(t_all[k]).max()
        assert np.abs(t_all[k] - (truth_i[k] + t_maps[k])).max() <= 1e-12 * s
        assert np.abs(t_maps[k] - (t_d[k] + t_a[k])).max() <= 1e-12 * max(np.abs(t_maps[k]).max(), 1e-300)


def test_maps_posed_as_colours_is_the_derivative_of_the_maps():
    """Central finite difference, accumulated in float64, of L = <gd, D> + <ga, A> on the translucent scene with respect to
    one Gaussian's depth colour d_i and its activated opacity, from oracle.draw on perturbed SORTED inputs (no re-sort;
    translucent, so no stop decision flips), against the per-Gaussian sums of oracle.draw_backward_f64's rows: within 1e-3.
    oracle.draw is fp32, so the steps are large -- which costs nothing: L is linear in d_i, and, every Gaussian entering a
    pixel once and alpha_i = o_i G_i carrying no cap, affine in one Gaussian's opacity: the central difference has no
    truncation error at any step, nor does the slope between any two opacities.  Steps: d_i +- 1; the opacity set to 0 and
    to 0.5 (every perturbed frame is checked to stay below the stop threshold in every pixel)."""
    import numpy as np

    import oracle
    from gs_testutil import _sum_by_id, aux_colours, robust_aux_grads, saturated_share

    of = _small_case(-4.0)
    assert saturated_share(of) == 0.0
    g, n = of.grid, of.scene.n
    _, gd, ga, n_masked = robust_aux_grads(of, 17)
    assert n_masked == 0
    gpad = of._padded_grad_maps(gd, ga).astype(np.float64)
    cols = aux_colours(of)
    _, gr, go, _ = of.aux_rows_f64(gd, ga)
    d_dep, d_opa = _sum_by_id(of.ids, gr[:, 0], n), _sum_by_id(of.ids, go, n)

    def L(c, o):
        out = oracle.draw(of.s_pos, c, o, of.s_cov, of.accum, g.padded_height, g.padded_width, g.focal_x, g.focal_y,
                          use_sh=False, fast=True)
        assert float(out[:, :, 1].max()) < 0.9995  # away from the stop threshold (alpha 0.9999): no decision flips
        return float((out.astype(np.float64) * gpad).sum())

    assert np.array_equal(L(cols, of.s_opa), float((of.aux_maps().astype(np.float64) * gpad).sum()))
    ok = of.opa_act < 0.5
    picks = set(np.argsort(-np.abs(d_dep) * ok)[:4]) | set(np.argsort(-np.abs(d_opa) * ok)[:4]) | \
        set(np.argsort(-np.bincount(of.ids, minlength=n) * ok)[:2])
    assert len(picks) >= 5
    for i in sorted(picks):
        rows = of.ids == i
        cp, cm = cols.copy(), cols.copy()
        cp[rows, 0] += 1.0
        cm[rows, 0] -= 1.0
        fd = (L(cp, of.s_opa) - L(cm, of.s_opa)) / 2.0
        assert abs(fd - d_dep[i]) <= 1e-3 * abs(d_dep[i]), ("depth colour", i, fd, d_dep[i])
        op, om = of.s_opa.copy(), of.s_opa.copy()
        op[rows], om[rows] = np.float32(0.5), np.float32(0.0)
        fd = (L(cols, op) - L(cols, om)) / 0.5
        assert abs(fd - d_opa[i]) <= 1e-3 * abs(d_opa[i]), ("opacity", i, fd, d_opa[i])


def test_depth_loss_f64_and_masked_count_helpers():
    """robust_aux_grads returns the number of masked PIXELS (what robust_grad_image counts) and zeroes all three maps there;
    depth_loss_f64 differentiates its own loss (central difference in double on measured pixels)."""
    import numpy as np

    from gs_testutil import depth_loss_f64, robust_aux_grads

    of = _small_case(0.0)
    gimg, gd, ga, n_masked = robust_aux_grads(of, 5)
    _, n_ref = of.robust_grad_image(np.ones(of.image.shape, np.float32))
    assert n_masked == n_ref > 0
    zero = (gd == 0) & (ga == 0) & (gimg == 0).all(axis=2)
    assert int(zero.sum()) == n_masked
    rng = np.random.default_rng(3)
    A = rng.uniform(0.02, 1.0, (24, 32))
    z = rng.uniform(0.3, 12.0, (24, 32))
    D = A * z * rng.uniform(0.7, 1.3, (24, 32))
    z[rng.uniform(size=z.shape) < 0.3] = np.nan
    z[0, :4] = (0.0, -1.0, np.inf, -np.inf)
    for mode in ("residual", "expected"):
        gdl, gal, loss, count, r, measured = depth_loss_f64(D, A, z, mode, 0.5, 0.25)
        valid = np.isfinite(z) & (np.nan_to_num(z, nan=0.0, posinf=0.0) > 0) & ((A >= 0.5) | (mode == "residual"))
        assert np.array_equal(measured, valid) and count == int(valid.sum())
        assert np.all(gdl[~valid] == 0) and np.all(gal[~valid] == 0)
        assert abs(loss - 0.25 * np.abs(r).sum()) < 1e-15
        for (y, x) in [tuple(p) for p in np.argwhere(valid)[:5]]:
            for arr, grad in ((D, gdl), (A, gal)):
                h = 1e-6
                p, m = arr.copy(), arr.copy()
                p[y, x] += h
                m[y, x] -= h
                args = (lambda q: (q, A, z)) if arr is D else (lambda q: (D, q, z))
                fd = (depth_loss_f64(*args(p), mode, 0.5, 0.25)[2] - depth_loss_f64(*args(m), mode, 0.5, 0.25)[2]) / (2 * h)
                assert abs(fd - grad[y, x]) <= 1e-6 * max(abs(grad[y, x]), 1.0), (mode, y, x, fd, grad[y, x])
