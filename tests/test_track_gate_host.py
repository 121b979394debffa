"""CPU tier of the median-gated tracking loss (include/gs_abi.h: gs_loss_track_gated_workspace_bytes, gs_loss_track_gated;
gs_train.GatedTrackLoss; gs_track.TrackOptions / Tracker.loss_plan / TrackResult): the symbols and their bindings, the
workspace size query, every refusal on fake pointers (each comes before anything is enqueued), the Python surface's defaults
and refusals, the Tracker's choice of the ungated path with the gate off, the kernels' resources from the built code object,
and the numpy reference of tests/track_gate_ref.py against a plain np.sort statement on the GPU tier's inputs.  No kernel is
launched."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1
FAKE = 1 << 40
H, W = 48, 64


def test_symbols_exist_and_are_bound():
    from gaussian import _lib

    for name in ("gs_loss_track_gated_workspace_bytes", "gs_loss_track_gated"):
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
        assert callable(getattr(_lib, name))
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    for name in ("size_t gs_loss_track_gated_workspace_bytes(", "int gs_loss_track_gated("):
        assert name in header
    assert _lib.lib.gs_abi_version() == 8  # additive: the version stays


def test_workspace_size_query():
    from gaussian import _lib

    q = _lib.gs_loss_track_gated_workspace_bytes
    sizes = [(1, 1), (7, 9), (48, 64), (187, 250), (480, 640), (1080, 1920), (2160, 3840), (4096, 4096)]
    got = [q(h, w) for h, w in sizes]
    for (h, w), b in zip(sizes, got):
        assert b % 256 == 0
        assert b >= 8 * h * w + 16 * -(-h * w // 1024) + 3 * 2 * 2048 * 4  # two residual maps, the rows, the select's counters
    assert got == sorted(got) and got[-1] > got[0]  # monotone in H * W
    assert q(64, 48) == q(48, 64)
    for bad in ((0, 64), (48, 0), (-1, 64), (48, -7), (0, 0)):
        assert q(*bad) == 0


def test_loss_rejects_bad_arguments_before_any_launch():
    from gaussian import _lib

    ws_bytes = _lib.gs_loss_track_gated_workspace_bytes(H, W)
    IMG, D, A, TI, TZ, GI, GD, GA, VAL, WS, RD, RC = (FAKE + i * (1 << 24) for i in range(12))

    def call(image=IMG, depth=D, alpha=A, timg=TI, trange=TZ, h=H, w=W, amin=0.5, cw=1.0, dw=1.0, kd=10.0, kc=0.0, fd=0.0,
             fc=0.0, couple=1, scale=1.0, gi=GI, gd=GD, ga=GA, val=VAL, rd=RD, rc=RC, ws=WS, nbytes=ws_bytes):
        return _lib.gs_loss_track_gated(image, depth, alpha, timg, trange, h, w, amin, cw, dw, kd, kc, fd, fc, couple, scale,
                                        gi, gd, ga, val, rd, rc, ws, nbytes, None)

    def refused(word, **kw):
        assert call(**kw) == GS_E_INVALID, kw
        msg = _lib.gs_last_error()
        assert b"gs_loss_track_gated" in msg and word in msg, (kw, msg)

    # every refusal of gs_loss_track
    for kw in ("image", "depth", "alpha", "timg", "gi", "gd", "ga"):
        refused(b"null", **{kw: None})
    for hw in ((0, W), (H, 0), (-1, W), (H, -3)):
        refused(b"empty", h=hw[0], w=hw[1])
    for kw, base in (("image", IMG), ("depth", D), ("alpha", A), ("timg", TI), ("trange", TZ), ("gi", GI), ("gd", GD),
                     ("ga", GA), ("rd", RD), ("rc", RC)):
        for off in (4, 8):
            refused(b"16-byte aligned", **{kw: base + off})  # the maps are walked float4 by float4
    for amin in (0.0, -0.5, float("nan")):
        refused(b"alpha_min", amin=amin)
    for bad in (-1.0, -1e-30, float("nan")):
        refused(b"weight", cw=bad)
        refused(b"weight", dw=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"scale", scale=bad)
    refused(b"workspace", ws=None)
    refused(b"workspace", ws=WS + 8)
    refused(b"workspace", nbytes=ws_bytes - 1)
    refused(b"workspace", nbytes=0)
    refused(b"values_out", val=VAL + 2)
    # and its own
    for bad in (-1.0, -1e-30, float("nan")):
        refused(b"floor", fd=bad)
        refused(b"floor", fc=bad)
    refused(b"NaN", kd=float("nan"))
    refused(b"NaN", kc=float("nan"))
    big = _lib.gs_loss_track_gated_workspace_bytes(4096, 4097)
    refused(b"2^24", h=4096, w=4097, nbytes=big)  # one row beyond 2^24 pixels
    refused(b"2^24", h=1, w=(1 << 24) + 1, nbytes=big)


def test_python_surface_defaults_and_refusals():
    import gs_track
    import gs_train

    with pytest.raises(RuntimeError, match="no CPU fallback"):  # HIP kernels
        gs_train.GatedTrackLoss(48, 64, 0.5, 1.0, 1.0, 10.0, 0.0, 0.0, 0.0, True, "cpu")
    o = gs_track.TrackOptions()
    assert (o.depth_gate_k, o.color_gate_k, o.depth_gate_floor, o.color_gate_floor, o.gate_couple) == (0.0, 0.0, 0.0, 0.0, True)
    names = list(gs_track.TrackOptions.__dataclass_fields__)
    assert names[-5:] == ["depth_gate_k", "color_gate_k", "depth_gate_floor", "color_gate_floor", "gate_couple"]  # trailing
    assert not o.gated()
    with pytest.raises(ValueError, match="depth_gate .* and depth_gate_k .* both gate the depth term: give one of them"):
        gs_track.TrackOptions(depth_gate=2.0, depth_gate_k=10.0).gated()
    with pytest.raises(ValueError, match="give one of them"):
        gs_track.Tracker.loss_plan(gs_track.TrackOptions(depth_gate=2.0, depth_gate_k=10.0), 48, 64)
    assert gs_track.TrackOptions(depth_gate=2.0, color_gate_k=3.0).gated()  # (a fixed depth gate beside a colour median gate)
    r = gs_track.TrackResult(rot=np.eye(3), tran=np.zeros(3), loss=0.0, iterations=0)
    assert r.inliers is None and r.medians is None  # the gate's report: None with the gate off


def test_tracker_selects_the_ungated_path_with_the_gate_off():
    """Tracker.loss_plan decides the loss object and the size of the per-iteration buffer from the options alone."""
    import gs_track
    import gs_train

    cls, args, nfloat = gs_track.Tracker.loss_plan(gs_track.TrackOptions(), 120, 160)
    assert cls is gs_train.TrackLoss and nfloat == 16  # a 64-byte read
    assert args == (120, 160, 0.5, 1.0 / 3.0, 1.0, 0.0)  # exactly what the Tracker gave TrackLoss before the gate existed
    cls, args, nfloat = gs_track.Tracker.loss_plan(gs_track.TrackOptions(depth_gate=2.0, depth_gate_k=-1.0), 120, 160)
    assert cls is gs_train.TrackLoss and nfloat == 16 and args[-1] == 2.0
    for kw in (dict(depth_gate_k=10.0), dict(color_gate_k=10.0), dict(depth_gate_k=10.0, color_gate_k=5.0)):
        o = gs_track.TrackOptions(depth_gate_floor=0.01, gate_couple=False, **kw)
        cls, args, nfloat = gs_track.Tracker.loss_plan(o, 120, 160)
        assert cls is gs_train.GatedTrackLoss and nfloat == 20
        assert args == (120, 160, 0.5, 1.0 / 3.0, 1.0, o.depth_gate_k, o.color_gate_k, 0.01, 0.0, False)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels():
    from test_kernel_resources import LIB, code_objects, kernel_metadata

    if not os.path.exists(LIB):
        pytest.skip("libgs_amd.so is not built")
    out = {}
    for elf in code_objects(open(LIB, "rb").read()):
        out.update(kernel_metadata(elf))
    return out


# LDS bytes: the residual and digit passes hold 2 x 2,048 32-bit counters (a counter holds a workgroup's whole share, so a
# frame that lands in one bin does not overflow), the digit and loss passes add the select's 48 bytes
GATE_KERNELS = {"track_gate_residual_kernelILb1EE": 16384, "track_gate_residual_kernelILb0EE": 16384,
                "track_gate_digit_kernelILi1EE": 16432, "track_gate_digit_kernelILi2EE": 16432,
                "track_gate_loss_kernelILb1EE": 112, "track_gate_loss_kernelILb0EE": 112, "track_gate_finalize_kernel": 512}


@pytest.mark.parametrize("part", list(GATE_KERNELS))
def test_track_gate_kernels_have_no_scratch(kernels, part):
    hits = [k for k in kernels if part in k]
    assert len(hits) == 1, (part, hits)
    k = kernels[hits[0]]
    assert k[".vgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0  # no scratch
    assert k[".group_segment_fixed_size"] == GATE_KERNELS[part], (k[".name"], k[".group_segment_fixed_size"])
    assert k[".vgpr_count"] <= 128  # at least four waves per SIMD


def test_no_new_kernel_name_collides_with_a_pinned_one(kernels):
    """The tests that pick a kernel by a substring of its name demand exactly one hit: the new kernels add none."""
    import re

    import test_kernel_resources
    from test_track_host import TRACK_KERNELS

    src = open(test_kernel_resources.__file__).read()
    pinned = set(re.findall(r'"([A-Za-z_0-9]*kernel[A-Za-z_0-9]*)"', src)) | set(TRACK_KERNELS) | {"track_loss_kernel"}
    new = [k for k in kernels if "track_gate_" in k]
    assert len(new) == len(GATE_KERNELS)
    for k in new:
        assert not any(p in k for p in pinned), k


# ---------------------------------------------------------------------------------------------------------------------
# what the issue computed on the GPU tier's inputs (k_d = k_c = 1.5, floors 0): (n_d, n_c) per size
EXPECTED_COUNTS = {(7, 9): (18, 35), (48, 64): (1075, 1538), (187, 250): (16778, 24024), (1080, 1920): (740572, 1057676)}


@pytest.mark.parametrize("case", range(4))
def test_reference_agrees_with_a_sort_on_the_gpu_tiers_inputs(case):
    """track_gate_ref selects the median on bit patterns; here the same contract with np.sort and plain boolean algebra, on
    the inputs of tests/test_gpu_track_gate.py -- and the non-vacuity of those inputs: each gate cuts 5 - 60 % of its set."""
    from track_gate_ref import gate_from_residuals, lower_median, residuals_f32
    from track_ref import ALPHA_MIN, LOSS_CASES, loss_inputs

    Hh, Ww, seed = LOSS_CASES[case]
    I, D, A, T, z = loss_inputs(Hh, Ww, seed)
    ra, rc, covered, meas = residuals_f32(I, D, A, T, z, ALPHA_MIN)
    va, vc = np.sort(ra[~np.isnan(ra)]), np.sort(rc[~np.isnan(rc)])
    assert (len(va), len(vc)) == EXPECTED_COUNTS[(Hh, Ww)]
    m_d, m_c = va[(len(va) - 1) // 2], vc[(len(vc) - 1) // 2]
    assert lower_median(va).tobytes() == m_d.tobytes() and lower_median(vc).tobytes() == m_c.tobytes()
    assert np.array_equal(np.isnan(ra), ~(covered & meas)) and np.array_equal(np.isnan(rc), ~covered)
    for couple in (True, False):
        g = gate_from_residuals(ra, rc, covered, meas, 1.5, 1.5, couple=couple)
        assert (g["n_d"], g["n_c"]) == EXPECTED_COUNTS[(Hh, Ww)]
        assert g["m_d"].tobytes() == m_d.tobytes() and g["m_c"].tobytes() == m_c.tobytes()
        t_d, t_c = np.float32(1.5) * m_d, np.float32(1.5) * m_c
        dmask = np.zeros((Hh, Ww), bool)
        cmask = np.zeros((Hh, Ww), bool)
        for y in range(Hh) if Hh * Ww < 4000 else ():  # pixel by pixel at the small sizes
            for x in range(Ww):
                if not covered[y, x]:
                    continue
                d_ok = bool(meas[y, x]) and ra[y, x] <= t_d
                dmask[y, x] = d_ok
                dropped = couple and bool(meas[y, x]) and not d_ok
                cmask[y, x] = (not dropped) and rc[y, x] <= t_c
        if Hh * Ww >= 4000:
            dmask = covered & meas & (np.nan_to_num(ra, nan=np.inf) <= t_d)
            cmask = covered & (np.nan_to_num(rc, nan=np.inf) <= t_c) & ~((covered & meas & ~dmask) if couple else False)
        assert np.array_equal(g["dmask"], dmask) and np.array_equal(g["cmask"], cmask)
        cut_d = 1.0 - dmask.sum() / g["n_d"]
        cut_c = 1.0 - (covered & (np.nan_to_num(rc, nan=np.inf) <= t_c)).sum() / g["n_c"]
        assert 0.05 <= cut_d <= 0.60 and 0.05 <= cut_c <= 0.60, (cut_d, cut_c)
    # the gates off: gs_loss_track's masks
    g = gate_from_residuals(ra, rc, covered, meas, 0.0, 0.0)
    assert np.array_equal(g["dmask"], covered & meas) and np.array_equal(g["cmask"], covered)


def test_reference_on_the_crafted_sets():
    from track_gate_ref import crafted_inputs, gate_from_residuals, low_bits, lower_median, powers_and_zeros, residuals_f32

    assert lower_median([]) == 0 and lower_median([3.0]) == 3.0 and lower_median([3.0, 1.0]) == 1.0
    assert lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0  # the lower of the two middle elements, not their mean
    n = 48 * 64
    for resid in (np.ones(n), powers_and_zeros(n), low_bits(n)):
        I, D, A, T, z = crafted_inputs(48, 64, resid)
        ra, rc, covered, meas = residuals_f32(I, D, A, T, z, 0.5)
        assert np.array_equal(ra.reshape(-1), np.asarray(resid, np.float32))  # exact by construction
        g = gate_from_residuals(ra, rc, covered, meas, 1.5, 0.0)
        assert g["m_d"] == np.sort(ra.reshape(-1))[(n - 1) // 2] and g["n_d"] == n
    bits = low_bits(n).view(np.uint32)
    assert len(set(bits >> 10)) == 1 and len(set(bits & 1023)) == 512  # only the last level tells them apart
    assert len(set(powers_and_zeros(n).view(np.uint32) >> 21)) == 24
