"""The catalogue of tests/frame_history.py is a valid input -- proven here on the oracle alone, as
tests/test_general_camera_host.py does for its cases --, and its histories contain every transition they are meant to
contain: tests/test_gpu_frame_history.py then asserts kernels and caches and never discovers on the device that a scene is
out of view, that a capacity was not what the history assumes, or that a transition was never rendered."""
import numpy as np
import pytest

import frame_history as FH

# FrameRenderer's thresholds, restated (the GPU tier compares them with the class's own)
LONG_SORT_FLAG_AT = LONG_LIST_FLAG_AT = 2_048
CULL_NEAR_SHIFT_PX, CULL_MAX_SHIFT_PX, CULL_MIN_GAIN = 0.5, 8.0, 0.65
HEADROOM = 1.25

# The transitions the histories must contain between them, line by line (frame_history.transitions computes what a history has).
REQUIRED = frozenset(
    # W x H shrinking and growing at unchanged scene, once for I and once for Tb
    [("size", a, b, m) for m in ("I", "Tb") for a, b in (("C1", "C2"), ("C2", "C1"), ("C2", "C3"), ("C3", "C2"),
                                                          ("C1", "C4"), ("C4", "C1"))] +
    # N shrinking and growing at unchanged size: the same address, the same N at another address, tiny, beyond the strip limit
    [("count", a, b) for a, b in (("A", "A2000"), ("A2000", "A"), ("A", "B"), ("B", "A"), ("A", "TINY"), ("TINY", "A"),
                                  ("A", "BIG"), ("BIG", "A"))] +
    # the colour dimension at unchanged camera, in both orders
    [("colour", a, b) for a, b in (("A", "SH2"), ("SH2", "SH3"), ("SH3", "A"), ("A", "SH3"))] +
    # all of I, Ia, T, Tab after each other
    [("mode", a, b) for a in ("I", "Ia", "T", "Tab") for b in ("I", "Ia", "T", "Tab") if a != b] +
    [("behind_an_open_T", m) for m in ("Tb", "Tab", "Tp")] +
    [("rest_near_mid_far_back",), ("rest_interrupted_near_mid_far_back",), ("camera_in_place",)] +
    [("behind_pile", x) for x in ("A", "SH2", "C2")] +
    [("grown_then_small",), ("overflowed_then_clean",)])


@pytest.mark.parametrize("scene,camera", FH.distinct_frames(), ids=lambda v: v)
def test_every_frame_of_the_catalogue_is_a_valid_input(scene, camera):
    of = FH.oracle_frame(scene, camera)
    lens = np.diff(of.accum)
    walk = int(FH.walk_lengths_f64(of).max())
    visible = float(of.mask.mean())
    line = (f"frame history case {scene} {camera}: visible {visible:.2f}, pairs {len(of.ids)}, longest list {int(lens.max())}, "
            f"longest walk {walk}")
    print(line)
    assert (int(of.mask.sum()) >= 1) if scene == "TINY" else (visible >= 0.3), line
    assert len(of.ids) > 0, line
    # no frame of any history may latch the segmented compositing, which is not promised to be bit-identical: the longest
    # WALK stays within LONG_LIST_FLAG_AT everywhere, also where the longest LIST does not
    assert walk <= LONG_LIST_FLAG_AT, line


@pytest.mark.parametrize("name", sorted(FH.HISTORIES))
def test_pair_counts_against_the_capacity_of_the_history(name):
    """Below the capacity the frame meets, except in the overflow steps: there above it (and where the history's renderer
    grows, the capacity it grows to is the one the later frames meet)."""
    h = FH.HISTORIES[name]
    cap = h.max_pairs
    for k, s in enumerate(h.steps):
        pairs = len(FH.oracle_frame(s.scene, FH.pose_name(s.camera)).ids)
        if k in h.overflow:
            assert pairs > cap, (name, k, s, pairs, cap)
            if h.grows:
                cap = int(pairs * HEADROOM) + 1024
        else:
            # (auto_grow="async" grows ahead of a frame that comes within 25 % of the capacity: none does)
            assert pairs * HEADROOM < cap, (name, k, s, pairs, cap)
    assert all(s.mode in FH.MODES for s in h.steps)
    assert not any(s.mode == "Tp" and s.colour_dim() != 3 for s in h.steps)
    assert bool(h.overflow) == bool(h.about & {"grow", "overflow"})


def test_lists_beyond_one_bucket_and_the_pile():
    longest = {fc: int(np.diff(FH.oracle_frame(*fc).accum).max()) for fc in FH.distinct_frames()}
    assert any(v > 64 for (s, _), v in longest.items() if FH.scene(s).rgb.shape[1] == 3)
    assert any(v > 64 for (s, _), v in longest.items() if FH.scene(s).rgb.shape[1] != 3)
    pile = FH.oracle_frame("PILE", "C1")
    lens, walk = np.diff(pile.accum), FH.walk_lengths_f64(pile)
    print("PILE: longest list", int(lens.max()), "longest walk", int(walk.max()))
    assert lens.max() > LONG_SORT_FLAG_AT and walk.max() <= LONG_LIST_FLAG_AT
    # ... and PILE is the only small scene that latches the long sort: what follows it in its history is flagged BY it
    for (s, c), v in longest.items():
        assert (v > LONG_SORT_FLAG_AT) == (s in ("PILE", "BIG")), (s, c, v)
    # BIG is on the strip side of the library's choice, every other scene on the table side
    assert FH.scene("BIG").n > 131_072 and all(FH.scene(s).n < 131_072 for s in FH.SCENES if s != "BIG")
    a, a2 = FH.scene("A"), FH.scene("A2000")
    assert a2.n == 2_000 and np.shares_memory(a.pos, a2.pos) and FH.scene("B").n == a.n and FH.scene("TINY").n == 37
    assert FH.scene("PILE").n == 2_000 + FH.PILE_COUNT and FH.scene("SH2").rgb.shape[1] == 27 and FH.scene("SH3").rgb.shape[1] == 48


def test_camera_shifts_fall_into_the_three_bands():
    """_camera_shift_px restated: C1near is a near pose, C1mid a dilated one, C1far beyond the cull -- against C1 and against
    the camera that precedes each of them in the histories (the renderer measures from the last inference frame)."""
    c1, near, mid, far = (FH.camera(n) for n in ("C1", "C1near", "C1mid", "C1far"))
    s_near, s_mid, s_far = (FH.camera_shift_px(c1, c) for c in (near, mid, far))
    print("shifts against C1:", s_near, s_mid, s_far)
    assert FH.camera_shift_px(c1, FH.camera("C1")) == 0.0
    assert 0.0 < s_near <= CULL_NEAR_SHIFT_PX < s_mid <= CULL_MAX_SHIFT_PX < s_far
    assert abs(s_near - 0.335) < 0.01 and abs(s_mid - 5.03) < 0.05
    assert CULL_NEAR_SHIFT_PX < FH.camera_shift_px(near, mid) <= CULL_MAX_SHIFT_PX
    assert FH.camera_shift_px(mid, far) > CULL_MAX_SHIFT_PX and FH.camera_shift_px(far, c1) > CULL_MAX_SHIFT_PX
    assert FH.camera_shift_px(c1, mid) <= CULL_MAX_SHIFT_PX  # (the viewer history: C1mid -> C1 is dilated again)
    for other in ("C2", "C3", "C4", "C5", "C6"):
        assert FH.camera_shift_px(c1, FH.camera(other)) > CULL_MAX_SHIFT_PX, other
    # C2 and C3 share a padded grid and differ in the crop; C4 is taller than wide
    from gs_geometry import TileGrid

    g2, g3 = (TileGrid(c.width, c.height, c.focal_x, c.focal_y) for c in (FH.camera("C2"), FH.camera("C3")))
    assert (g2.padded_width, g2.padded_height) == (g3.padded_width, g3.padded_height) == (64, 48)
    assert (g2.width, g2.height) != (g3.width, g3.height)


def test_the_cull_pays_on_the_resting_frame():
    """The resting histories rely on the renderer KEEPING the cull on (A, C1): an estimate of what a culled repeat of that
    frame emits, well below CULL_MIN_GAIN of the pairs."""
    for cam in ("C1", "C1near", "C1mid"):
        share = FH.cull_emitted_share_f64(FH.oracle_frame("A", cam))
        print("A", cam, "culled repeat emits", round(share, 3))
        assert share < CULL_MIN_GAIN - 0.1, (cam, share)


def test_the_histories_cover_every_transition():
    covered = set().union(*(FH.transitions(h) for h in FH.HISTORIES.values()))
    missing = REQUIRED - covered
    assert not missing, sorted(missing)
    # the literal table, so that a change of REQUIRED is a change of this file too
    assert len(REQUIRED) == 12 + 8 + 4 + 12 + 3 + 3 + 3 + 2
    for line in (("size", "C2", "C3", "Tb"), ("count", "A", "A2000"), ("count", "BIG", "A"), ("colour", "SH3", "A"),
                 ("mode", "Tab", "Ia"), ("behind_an_open_T", "Tp"), ("rest_interrupted_near_mid_far_back",),
                 ("camera_in_place",), ("behind_pile", "C2"), ("grown_then_small",), ("overflowed_then_clean",)):
        assert line in REQUIRED and line in covered, line
    # every history is about something on the list, and the seeded walks repeat themselves
    for h in FH.HISTORIES.values():
        assert FH.transitions(h) or h.about or h.name.startswith("shuffle"), h.name
    assert FH._shuffled(101, 16) == FH.HISTORIES["shuffle_1"].steps
