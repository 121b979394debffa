"""CPU tier of GS_FRAME_CULL_REPEAT (include/gs_abi.h): an occlusion-culled frame that repeats the previous forward is issued
without the five gated launches of its second pass.

Through the library, on fake pointers and without a device: which descriptors enqueue the gated launches
(gs_frame_cull_second_pass), the refusal of the flag together with GS_FRAME_CULL_DILATE, the flag's value and the frame flags'
bits.  On the CPU model of the trim rule (tests/cull_trim_ref.py): the invariant the flag rests on -- a frame trimmed by the
cuts of a full walk at the same pose and scene raises no run-past, and leaves the cut table it read."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from cull_trim_ref import TrimModel, crafted_camera, crafted_scene, faded, moved_out
from gs_scene import make_camera, make_scene
from gs_testutil import fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1


def _lib():
    from gaussian import _lib

    return _lib


def _frame(flags=0, training=0, method=2, n=1000, **kw):
    """An inference descriptor of the strip variant (GS_FRAME_STRIP_BIN: the fake scene is small) unless `flags` says otherwise."""
    L = _lib()
    f = fake_frame(training=training, N=n, **kw)
    f.tile_culling_method = method
    if method == 0:
        f.thresh = 4.0  # "dist": a squared distance
    f.flags |= flags
    if not (flags & (L.GS_FRAME_TABLE_BIN | L.GS_FRAME_SLICE_SORT)):
        f.flags |= L.GS_FRAME_STRIP_BIN
    return f


def _second_pass(f):
    L = _lib()
    out, culled = C.c_int32(-1), C.c_int32(-1)
    rc = L.gs_frame_cull_second_pass(C.byref(f), C.byref(out))
    assert L.gs_frame_is_occlusion_culled(C.byref(f), C.byref(culled)) == 0
    return rc, out.value, culled.value


def test_flag_is_the_next_free_bit_and_the_abi_is_additive():
    L = _lib()
    assert L.GS_FRAME_CULL_REPEAT == 65536 == 2 * L.GS_FRAME_DEVICE_POSE
    assert L.gs_abi_version() == 8
    assert "gs_frame_cull_second_pass" in L.EXPORTS and L.lib.gs_frame_cull_second_pass is not None
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    assert re.search(r"#define GS_FRAME_CULL_REPEAT 65536\b", header) and re.search(r"#define GS_ABI_VERSION 8\b", header)


def test_every_frame_flag_has_its_own_bit():
    """In the header and in the ctypes mirror: the same names, the same values, each a single bit, no bit twice."""
    L = _lib()
    header = open(os.path.join(ROOT, "include", "gs_abi.h")).read()
    in_header = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (GS_FRAME_[A-Z_]+) (\d+)\b", header, re.M)}
    in_python = {k: v for k, v in vars(L).items() if k.startswith("GS_FRAME_") and isinstance(v, int)}
    assert in_header == in_python and len(in_header) == 17
    values = sorted(in_header.values())
    assert all(v > 0 and v & (v - 1) == 0 for v in values) and len(set(values)) == len(values)
    assert values == [1 << k for k in range(17)]  # no gap below the new flag: it IS the next free bit


def test_which_descriptors_enqueue_the_gated_launches():
    """gs_frame_cull_second_pass: 1 for a culled frame without the flag, 0 with it -- and 0 wherever GS_FRAME_OCCLUSION_CULL is
    ignored (no second pass exists there), flag or no flag."""
    L = _lib()
    CULL, REPEAT = L.GS_FRAME_OCCLUSION_CULL, L.GS_FRAME_CULL_REPEAT
    # culled: inference, prob / prob2 listing, strip variant
    for method in (1, 2):
        assert _second_pass(_frame(CULL, method=method)) == (0, 1, 1)
        assert _second_pass(_frame(CULL | REPEAT, method=method)) == (0, 0, 1)
    # a scene large enough to take the strip variant by itself
    big = fake_frame(training=0, N=200_000)
    big.flags |= CULL
    assert _second_pass(big) == (0, 1, 1)
    big.flags |= REPEAT
    assert _second_pass(big) == (0, 0, 1)
    # dilated cuts keep their second pass
    assert _second_pass(_frame(CULL | L.GS_FRAME_CULL_DILATE)) == (0, 1, 1)
    assert _second_pass(_frame(CULL | L.GS_FRAME_CULL_DILATE | L.GS_FRAME_CULL_DILATE_NEAR)) == (0, 1, 1)
    # not culled: nothing to enqueue, with or without the flag
    ignored = [dict(flags=0), dict(flags=CULL, training=1), dict(flags=CULL | L.GS_FRAME_EMIT_SORTED_KEYS),
               dict(flags=CULL | L.GS_FRAME_LONG_LISTS), dict(flags=CULL | L.GS_FRAME_SERIAL_LONG_LISTS),
               dict(flags=CULL, method=0), dict(flags=CULL | L.GS_FRAME_TABLE_BIN), dict(flags=CULL | L.GS_FRAME_SLICE_SORT)]
    for kw in ignored:
        for extra in (0, REPEAT):
            kw2 = dict(kw, flags=kw["flags"] | extra)
            assert _second_pass(_frame(**kw2)) == (0, 0, 0), kw2
    # (the table variant by the library's own choice: a small scene without GS_FRAME_STRIP_BIN)
    small = fake_frame(training=0)
    small.flags |= CULL | REPEAT
    assert _second_pass(small) == (0, 0, 0)
    # sort_mode 0 / 1: the radix variants
    for mode in (0, 1):
        f = _frame(CULL | REPEAT)
        f.sort_mode = mode
        assert _second_pass(f) == (0, 0, 0)


def test_the_flag_with_dilated_cuts_is_refused_with_its_reason():
    """By the query and by validate (reached through gs_frame_binning_variant, which launches nothing), whether or not the
    frame is culled at all: the two flags contradict each other."""
    L = _lib()
    CULL, REPEAT, DILATE = L.GS_FRAME_OCCLUSION_CULL, L.GS_FRAME_CULL_REPEAT, L.GS_FRAME_CULL_DILATE
    for kw in (dict(flags=CULL | REPEAT | DILATE), dict(flags=CULL | REPEAT | DILATE | L.GS_FRAME_CULL_DILATE_NEAR),
               dict(flags=REPEAT | DILATE), dict(flags=CULL | REPEAT | DILATE, training=1)):
        f = _frame(**kw)
        out = C.c_int32(-7)
        assert L.gs_frame_cull_second_pass(C.byref(f), C.byref(out)) == GS_E_INVALID and out.value == -7
        why = L.gs_last_error().decode()
        assert "GS_FRAME_CULL_REPEAT" in why and "GS_FRAME_CULL_DILATE" in why and "moved" in why, why
        assert L.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
        assert "GS_FRAME_CULL_REPEAT" in L.gs_last_error().decode()
    # each flag alone validates
    for flags in (CULL | REPEAT, CULL | DILATE, REPEAT):
        assert L.gs_frame_binning_variant(C.byref(_frame(flags))) == 4
    # null arguments
    assert L.gs_frame_cull_second_pass(None, C.byref(C.c_int32())) == GS_E_INVALID
    assert L.gs_frame_cull_second_pass(C.byref(_frame(CULL)), None) == GS_E_INVALID


# ------------------------------------------------------------------------------------------ the invariant, on the CPU model
def _random_case(seed):
    """A small opaque scene (hundreds of Gaussians per tile: the tiles saturate, the cut table is not all GS_NO_CUT), seeded;
    ten tiles per tile row = one whole strip and a ragged one."""
    rng = np.random.default_rng(1000 + seed)
    w, h = 160, 48 + 16 * int(rng.integers(0, 3))
    scene = make_scene(int(rng.integers(4000, 9000)), w, h, seed=100 + seed)
    scene.opa += np.float32(rng.uniform(2.0, 5.0))
    return scene, make_camera(w, h, yaw_deg=float(rng.uniform(-20, 20)))


CASES = {"crafted": lambda: (crafted_scene(), crafted_camera()),
         "crafted, no wall": lambda: (crafted_scene(wall=False), crafted_camera()),
         "faded": lambda: (faded(crafted_scene()), crafted_camera()),
         "moved out": lambda: (moved_out(crafted_scene()), crafted_camera()),
         "crafted, yawed": lambda: (crafted_scene(), crafted_camera(2.0))}
CASES.update({f"random {k}": (lambda k=k: _random_case(k)) for k in range(20)})


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_repeated_frame_raises_no_run_past(case):
    """Frame 1 walks the full lists and leaves its cuts; frame 2, the same pose and scene trimmed by them, stops every tile
    that has a cut at the Gaussian that set it: no tile ends live, none composites behind its cut, the image is frame 1's
    bit for bit -- and the cut table frame 2 leaves is the one it read, so frame 3 is frame 2 again.  For the model's own stop
    steps and for the device's (a liveness test in front of every 8th Gaussian)."""
    scene, cam = CASES[case]()
    m = TrimModel(scene, cam)
    full = m.image(m.lists)
    for live_every in (1, 8):
        s1 = m.stop_steps(m.lists, live_every)
        c1 = m.cuts(m.lists, s1)
        l2 = m.trimmed_lists(c1)
        s2 = m.stop_steps(l2, live_every)
        assert not m.ends_live(l2, s2, c1) and not m.past_cut(l2, s2, c1), (case, live_every)
        assert np.array_equal(m.cuts(l2, s2), c1), (case, live_every)
        assert np.array_equal(m.image(l2), full), (case, live_every)
    if case.startswith("random"):  # (not vacuous: tiles saturate, and the trim drops pairs)
        assert (c1 != np.uint32(0xFFFFFFFF)).sum() > m.T // 2 and m.pairs(l2) < m.pairs(m.lists), (case, m.pairs(l2), m.pairs(m.lists))
