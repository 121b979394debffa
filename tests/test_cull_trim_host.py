"""CPU tier: the crafted scene of tests/cull_trim_ref.py does what tests/test_gpu_cull_exact.py needs it to do -- so that the
GPU test cannot pass vacuously.

An occlusion-culled frame's trimmed tile list is the prefix {depth <= cut} plus the interior extras of runs that kept their
ends.  The scene reaches a tile -- (3, 3) -- that leaves its prefix, composites extras (the wall) WITHOUT three Gaussians that
lie in front of them (trimmed: they are inside that tile alone), and saturates there: no tile that has a cut ends live, so a
fallback that only looks for live ends raises nothing, and the image is wrong by 0.93.  The tiles that differ are among those
whose last composited Gaussian lies behind their cut, which is what the compositing kernel tests.

Every property is pinned for the model's own stop steps and for the device's (a liveness test in front of every 8th
Gaussian: ``live_every``), under the plain cut table and under both dilation factors."""
import functools

import numpy as np
import pytest

from cull_trim_ref import (BLOCK, DILATE, DILATE_NEAR, NO_CUT, OCC, SMALL, SMALL_PX, SMALL_TILE, TrimModel, crafted_camera,
                           crafted_scene, faded, moved_out)

EDITS = {"fade": faded, "move": moved_out}


@functools.lru_cache(maxsize=None)
def _frames12(live_every, wall=True):
    """(model of the unedited scene, frame 1's cuts, frame 2's trimmed lists, frame 2's stop steps and cuts)"""
    m = TrimModel(crafted_scene(wall), crafted_camera())
    s1 = m.stop_steps(m.lists, live_every)
    c1 = m.cuts(m.lists, s1)
    l2 = m.trimmed_lists(c1)
    s2 = m.stop_steps(l2, live_every)
    return m, c1, l2, s2, m.cuts(l2, s2)


def _depth(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


@pytest.mark.parametrize("live_every", [1, 8])
def test_frames_1_and_2(live_every):
    """(a) 1,299 pairs; the cuts are the occluder's (~2.27) on the block and the wall's (~8.96) everywhere else; frame 2 drops
    exactly the three small Gaussians' pairs, and its image and cuts are frame 1's bit for bit."""
    m, c1, l2, s2, c2 = _frames12(live_every)
    assert m.pairs(m.lists) == 1299
    d1 = _depth(c1).reshape(m.nty, m.ntx)
    for r in range(m.nty):
        for c in range(m.ntx):
            lo, hi = (2.25, 2.30) if (r, c) in BLOCK else (8.9, 9.0)
            assert lo < d1[r, c] < hi, (r, c, d1[r, c])
    assert m.pairs(l2) == 1299 - 3
    t = m.tile(*SMALL_TILE)
    assert sorted(set(m.lists[t]) - set(l2[t])) == list(range(SMALL.start, SMALL.stop))
    assert all(len(a) == len(b) for k, (a, b) in enumerate(zip(m.lists, l2)) if k != t)
    assert np.array_equal(m.image(l2), m.image(m.lists))
    assert np.array_equal(c2, c1)
    assert not m.ends_live(l2, s2, c1) and not m.past_cut(l2, s2, c1)  # the unchanged scene: neither rule fires (control)


@pytest.mark.parametrize("live_every", [1, 8])
@pytest.mark.parametrize("shift_px", [0.0, 0.3, 2.0])
@pytest.mark.parametrize("edit", sorted(EDITS))
def test_the_edited_scene_saturates_past_its_cut(edit, shift_px, live_every):
    """(b) - (e): after the edit -- at the recorded pose with the plain and both dilated tables, a third and two pixels away
    with the dilated ones -- no tile that has a cut ends live, tile (3, 3) is wrong by more than 0.5, nothing outside it
    differs, and every differing tile composited a Gaussian behind its cut."""
    m, _, _, _, c2 = _frames12(live_every)
    me = TrimModel(EDITS[edit](crafted_scene()), crafted_camera(shift_px))
    full = me.image(me.lists)
    for factor in ([None] if shift_px == 0.0 else []) + [DILATE, DILATE_NEAR]:
        cut = c2 if factor is None else m.dilate(c2, factor)
        small_d = _depth(me.dbits[SMALL])
        assert (_depth(cut[m.tile(*SMALL_TILE)]) < small_d).all(), "the small Gaussians are trimmed"  # 2.27 / 3.13 / 2.56 < 4.28
        l3 = me.trimmed_lists(cut)
        assert not set(l3[m.tile(*SMALL_TILE)]) & set(range(SMALL.start, SMALL.stop))
        s3 = me.stop_steps(l3, live_every)
        assert not me.ends_live(l3, s3, cut), (factor, "(b)")
        diff = np.abs(me.image(l3) - full).max(axis=2)
        differing = me.tile_of_pixels(diff > 0)
        r, c = SMALL_TILE
        assert diff[16 * r:16 * r + 16, 16 * c:16 * c + 16].max() > 0.5 and differing == {SMALL_TILE}, (factor, "(c)")
        past = me.past_cut(l3, s3, cut)
        assert differing <= past, (factor, "(d)")
        if factor is None:
            assert past == set(BLOCK)  # (the plain table: the whole block composites the wall behind its ~2.27)
        print(edit, shift_px, live_every, factor, "max diff", diff.max(), "pixels", int((diff > 0).sum()), "past", sorted(past))


@pytest.mark.parametrize("live_every", [1, 8])
def test_frame_4_is_culled_again_and_shows_the_small_gaussians(live_every):
    """Frame 3 is rendered from the full lists and leaves ITS cuts; frame 4, trimmed by them, is exact without a fallback, and
    pixel (56, 56) shows the small Gaussians (red)."""
    me = TrimModel(faded(crafted_scene()), crafted_camera())
    s3 = me.stop_steps(me.lists, live_every)
    c3 = me.cuts(me.lists, s3)
    l4 = me.trimmed_lists(c3)
    s4 = me.stop_steps(l4, live_every)
    img = me.image(l4)
    assert np.array_equal(img, me.image(me.lists)) and np.array_equal(me.cuts(l4, s4), c3)
    assert not me.past_cut(l4, s4, c3)
    assert (c3 != NO_CUT).all()  # (every tile saturates on the wall: a valid table, though nothing lies behind it to trim)
    assert img[SMALL_PX[1], SMALL_PX[0], 0] > 0.9


@pytest.mark.parametrize("live_every", [1, 8])
def test_control_without_the_wall_the_tile_ends_live(live_every):
    """The same edit without the wall: the block's tiles run out of Gaussians with live pixels, which the rule `a tile with a
    cut ended live` has always caught -- the frame is rendered from the full lists, no difference."""
    m, c1, l2, s2, c2 = _frames12(live_every, wall=False)
    assert np.array_equal(m.image(l2), m.image(m.lists)) and np.array_equal(c2, c1) and m.pairs(l2) == m.pairs(m.lists) - 3
    me = TrimModel(faded(crafted_scene(wall=False)), crafted_camera())
    l3 = me.trimmed_lists(c2)
    s3 = me.stop_steps(l3, live_every)
    assert me.tile_of_pixels(np.abs(me.image(l3) - me.image(me.lists)).max(axis=2) > 0) == {SMALL_TILE}
    assert SMALL_TILE in me.ends_live(l3, s3, c2)
