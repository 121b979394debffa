"""GPU tier of the compact phase of the rgb inference compositing kernel (raster_fwd_body.h, raster_forward_kernel<3, true,
false, ...>): once at most 128 of a tile's 256 pixels are alive, the wave writes the stopped ones out, hands the live ones
over through LDS and composites two pixels per lane instead of four.

GS_FWD_COMPACT=0 in the environment (read per frame) keeps every tile in the full layout.  Both settings must render the
same bits, so every comparison here is torch.equal between two runs of the same library; where a tile compacted is read from
FrameRenderer.tile_compact_steps() (gs_frame_debug_tile_compact), and every test asserts that the regime it is about was
really crossed.

Scenes (camera: make_camera(W, H)): 500 opaque Gaussians (opacity logit 6, sigma ~ 2.5 px, z in [2, 3]) over the middle 80 %
of the width in front of 1,500 translucent ones (logit -2, sigma ~ 3 px, z in [4, 8]) everywhere, and 40 opaque ones in front
of the left ten columns of tile (1, 1), which therefore compacts inside its first chunk of 64.  Frames: 64 x 48 and 50 x 37
(12 tiles; the second is padded and cropped).  A float64 restatement of the walk on the oracle's lists gives, for seeds 1 / 2:
64 x 48: 11 / 9 tiles compact, at steps 24 - 224, and walk 150 - 450 further steps; 50 x 37: 8 / 8 compact.  In the cropped
frame the opaque band ends 12 pixels inside the padded frame, so the recipe alone lets none of the six tiles of the outer
columns compact (6 of 12); two more opaque patches over the outer tiles of the middle row make it 8, and those two tiles lie
half outside the crop: their hand-over flushes pixels that the crop drops and the padded image keeps.  The four corner tiles
never compact.  Lists reach 608 / 974 pairs (below the 1,024 asked for)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gaussian import _lib
from gs_frame import FrameRenderer
from gs_scene import Scene, make_camera
from gs_testutil import OracleFrame, to_torch

pytestmark = pytest.mark.gpu

MAX_PAIRS = 1 << 15
SIZES = [(64, 48), (50, 37)]
CHUNK = 64
CULL, REPEAT = _lib.GS_FRAME_OCCLUSION_CULL, _lib.GS_FRAME_CULL_REPEAT


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _copy(f, flags_on=0):
    """A copy of the rgb inference descriptor `f` with a fresh image (returned with it) and more flags."""
    g = _lib.GsFrameDP()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(_lib.GsFrameDP))
    g.flags |= flags_on
    image = torch.full((g.height, g.width, 3), -7.0, device=torch.device("cuda", torch.cuda.current_device()))
    g.image = image.data_ptr()
    return g, (image,)


def _counters(f, tag):
    """(visible, pairs, overflow, ran_past) of the last forward on f's workspace (synchronises)."""
    host = torch.zeros(_lib.GS_STATS_TAGGED_N, dtype=torch.int64).pin_memory()
    _lib.check(_lib.gs_frame_stats_tagged_async(C.byref(f), tag, host.data_ptr(), _stream()), "gs_frame_stats_tagged_async")
    torch.cuda.synchronize()
    h = host.tolist()
    assert int(h[11]) & 0xffffffff == tag
    return int(h[0]), int(h[1]), int(h[2]), int(h[10])


def _gaussians(rng, n, W, H, u_half, sigma_px, z_lo, z_hi, logit, u_mid=0.0, v_mid=0.0, v_half=None):
    """n Gaussians with centres uniform over the screen rectangle (u_mid +- u_half, v_mid +- v_half), in pixels from the
    centre, pixel sigma ~ sigma_px, depth in [z_lo, z_hi], opacity logit `logit`, random rotation and colour."""
    fx = 0.75 * W
    v_half = H / 2 if v_half is None else v_half
    z = rng.uniform(z_lo, z_hi, n)
    u = u_mid + rng.uniform(-u_half, u_half, n)
    v = v_mid + rng.uniform(-v_half, v_half, n)
    pos = np.stack([u / fx * z, v / fx * z, z], 1)
    scale = (sigma_px * z / fx)[:, None] * rng.uniform(0.6, 1.4, (n, 3))
    return pos, rng.normal(size=(n, 4)), scale, np.full(n, float(logit)), rng.normal(0.0, 1.0, (n, 3))


def _join(parts) -> Scene:
    return Scene(*(np.concatenate(a).astype(np.float32) for a in zip(*parts)))


@functools.lru_cache(maxsize=None)
def _scene(W, H, seed) -> Scene:
    """The recipe of the module docstring (cached, never modified)."""
    rng = np.random.default_rng(seed)
    parts = [_gaussians(rng, 500, W, H, 0.8 * W / 2, 2.5, 2.0, 3.0, 6.0),
             _gaussians(rng, 1500, W, H, W / 2 + 8, 3.0, 4.0, 8.0, -2.0),
             # (padded frames are 64 x 48 for both sizes: tile (1, 1) spans -16 .. 0 x -8 .. 8 pixels from the centre)
             _gaussians(rng, 40, W, H, 5.0, 3.5, 1.0, 1.5, 6.0, u_mid=-11.0, v_mid=0.0, v_half=8.0)]
    if W % 16:
        # the cropped frame: the band ends 12 pixels inside the padded frame, so no tile of the outer columns would compact.
        # Two more opaque patches, in the band's depth range, over the outer tiles of the middle row -- (0, 1) and (3, 1),
        # padded columns 2 .. 16 and 48 .. 62, half of them outside the crop: their early flush writes pixels the crop drops
        parts += [_gaussians(rng, 70, W, H, 7.0, 2.5, 2.0, 3.0, 6.0, u_mid=um, v_mid=0.0, v_half=8.0) for um in (-23.0, 23.0)]
    return _join(parts)


@functools.lru_cache(maxsize=None)
def _oracle_image(W, H, seed):
    return OracleFrame(_scene(W, H, seed), make_camera(W, H)).image


def _run(gpu, monkeypatch, scene, cam, compact, **renderer_args):
    """One forward of a fresh renderer with the compact phase on (the default: the variable unset) or off -> what it left."""
    if compact:
        monkeypatch.delenv("GS_FWD_COMPACT", raising=False)
    else:
        monkeypatch.setenv("GS_FWD_COMPACT", "0")
    args = dict(max_pairs=MAX_PAIRS, auto_grow=False, force_strips=True, occlusion_cull=False, scene_pack=False)
    args.update(renderer_args)
    r = FrameRenderer(gpu, **args)
    image, _ = r.forward(*to_torch(scene, gpu), cam)
    st = r.stats()
    assert r.binning_variant() == "strip" and st.overflow == 0
    out = dict(image=image.clone(), stats=st, cost=r.tile_cost().clone(), cuts=r.cut_table().clone(),
               at=r.tile_compact_steps().clone(), renderer=r)
    # the same frame once more at the library level with the padded image requested together with the cropped one
    f, (img2,) = _copy(r._frame)
    padded = torch.full((cam_padded(cam)[1], cam_padded(cam)[0], 3), -7.0, device=gpu)
    f.image_padded = padded.data_ptr()
    _lib.check(_lib.gs_frame_forward(C.byref(f), _stream()), "gs_frame_forward")
    torch.cuda.synchronize()
    out.update(image2=img2, padded=padded, at2=r.tile_compact_steps().clone())
    return out


def cam_padded(cam):
    return (cam.width + 15) // 16 * 16, (cam.height + 15) // 16 * 16


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_everything(a, b):
    """Images (NaNs compared by their bits), padded images, counters, tile costs and cut tables of two runs."""
    assert torch.equal(_bits(a["image"]), _bits(b["image"]))
    assert torch.equal(_bits(a["image2"]), _bits(b["image2"])) and torch.equal(_bits(a["image2"]), _bits(a["image"]))
    assert torch.equal(_bits(a["padded"]), _bits(b["padded"]))
    assert a["stats"] == b["stats"], (a["stats"], b["stats"])
    assert torch.equal(a["cost"], b["cost"]), (a["cost"], b["cost"])
    assert torch.equal(a["cuts"], b["cuts"])
    assert bool((b["at"] == -1).all()) and bool((b["at2"] == -1).all())  # no tile compacts with GS_FWD_COMPACT=0
    assert torch.equal(a["at"], a["at2"])


# ------------------------------------------------------------------------------------- 1, 2: compact equals full
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_compact_equals_full_and_the_regimes_were_crossed(gpu, monkeypatch, size, seed):
    """Default against GS_FWD_COMPACT=0: image, padded image, stats(), tile costs and cut table bit for bit; the default image
    within 5e-5 of the oracle; and from tile_compact_steps(): enough tiles compacted, one inside its first chunk and one in a
    later chunk, every one of them at least a whole chunk in front of its walk's end, and in the 50 x 37 frame one never
    (there, two of the tiles that compact lie half outside the crop)."""
    W, H = size
    scene, cam = _scene(W, H, seed), make_camera(W, H)
    on = _run(gpu, monkeypatch, scene, cam, True)
    off = _run(gpu, monkeypatch, scene, cam, False)
    at, cost = on["at"].cpu().numpy(), on["cost"].cpu().numpy()
    print(f"{W}x{H} seed {seed}: compacted at {at.tolist()}, walked {cost.tolist()}, M = {on['stats'].pairs}")
    _same_everything(on, off)
    err = float(np.abs(on["image"].cpu().numpy() - _oracle_image(W, H, seed)).max())
    assert err < 5e-5, err
    did = at != -1
    assert len(at) == 12
    assert did.sum() >= 8, at
    if size == (50, 37):
        assert did.sum() < 12 and did[4] and did[7], at  # (a corner tile never does; the two outer tiles of the middle row do)
    assert (at[did] < CHUNK).any() and (at[did] >= CHUNK).any(), at
    assert (at[did] % 8 == 0).all() and (cost[did] >= at[did] + CHUNK).all(), (at, cost)


# ------------------------------------------------------------------------------------- 3: exactly at the threshold
TARGET = (1, 1)  # the crafted tile: pixels 16 .. 31 x 16 .. 31 of the 64 x 48 frame
SLAB_SIGMA = 80.0
SLAB_ANGLE = np.deg2rad(33.0)


def _slab_scene(shift, background, unit_colour=False) -> Scene:
    """A three-deep stack of opaque Gaussians much larger than the tile, centred `shift` pixels from the far corner of the
    target tile along SLAB_ANGLE; five Gaussians of opacity 6e-6 behind it, so that the tile's first liveness test behind
    the stack (step 8) sees the stack's live set; then `background` translucent Gaussians."""
    W, H = 64, 48
    rng = np.random.default_rng(5)
    fx = 0.75 * W
    cx = 31.5 - 32.0 - shift * np.cos(SLAB_ANGLE)
    cy = 31.5 - 24.0 - shift * np.sin(SLAB_ANGLE)
    z = np.array([1.0, 1.01, 1.02, 1.1, 1.2, 1.3, 1.4, 1.5])
    u = np.array([cx] * 3 + [-8.0] * 5)
    v = np.array([cy] * 3 + [0.0] * 5)
    pos = np.stack([u / fx * z, v / fx * z, z], 1)
    scale = (SLAB_SIGMA * z / fx)[:, None] * np.array([[1.0, 0.8, 0.9]])
    quat = np.tile(np.array([[0.9, 0.1, -0.2, 0.35]]), (8, 1))
    opa = np.array([6.0] * 3 + [-12.0] * 5)
    rgb = rng.normal(0.0, 1.0, (8, 3))
    parts = [(pos, quat, scale, opa, rgb)]
    if background:
        parts.append(_gaussians(rng, background, W, H, W / 2 + 8, 3.0, 4.0, 8.0, -2.0))
    sc = _join(parts)
    if unit_colour:
        sc.rgb[:] = 30.0  # sigmoid = 1.0f: the oracle's image is then 1 - T
    return sc


def _oracle_live(shift):
    """(live pixels of the target tile behind the stack and its five followers, margin): from the oracle's image of those
    eight Gaussians with unit colours, sum w = 1 - T; margin = the smallest |T - 1e-4| over the tile's pixels."""
    of = OracleFrame(_slab_scene(shift, 0, unit_colour=True), make_camera(64, 48))
    tx, ty = TARGET
    t = 1.0 - of.padded[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16, 0].astype(np.float64)
    return int((t > 1e-4).sum()), float(np.abs(t - 1e-4).min())


@functools.lru_cache(maxsize=None)
def _shifts():
    """Shifts at which the oracle counts exactly 1, exactly 128 and 129 .. 140 live pixels, each decided with a margin of
    3e-7 in T -- five times the fp32 spacing of the image value 1 - T it is read from; the kernel's own T differs from the
    oracle's by some 1e-9 there (three factors 1 - alpha ~ 0.046, each a few 1e-6 relative) -- found by a sweep, not by
    construction."""
    found = {}
    for shift in np.arange(24.0, 44.0, 0.05):
        live, margin = _oracle_live(float(shift))
        key = "one" if live == 1 else "at" if live == 128 else "above" if 129 <= live <= 140 else None
        if key and key not in found and margin > 3e-7:
            found[key] = (float(shift), live)
    assert set(found) == {"one", "at", "above"}, found
    return found


@pytest.mark.parametrize("which", ["one", "at", "above"])
def test_tiles_exactly_at_the_threshold(gpu, monkeypatch, which):
    """1 and 128 live pixels at the first test behind the stack: the tile compacts there (step 8).  129 or more: it stays
    full until more pixels have died.  Everything equals the GS_FWD_COMPACT=0 run."""
    shift, live = _shifts()[which]
    scene, cam = _slab_scene(shift, 400), make_camera(64, 48)
    on = _run(gpu, monkeypatch, scene, cam, True)
    off = _run(gpu, monkeypatch, scene, cam, False)
    _same_everything(on, off)
    views = on["renderer"].debug_views()
    t = TARGET[1] * 4 + TARGET[0]
    start, end = (int(x) for x in views["tile_ranges"].cpu().numpy().reshape(-1, 2)[t])
    assert sorted(views["sorted_ids"].cpu().numpy()[start:start + 8].tolist()) == list(range(8)) and end - start >= 8 + 16
    at = int(on["at"][t])
    print(f"{which}: shift {shift:.2f}, oracle live {live}, compacted at {at}, walked {int(on['cost'][t])} of {end - start}")
    if which == "above":
        assert at > 8, at  # (not at the stack's test; -1, never, would fail too: the background kills the rim's pixels)
    else:
        assert at == 8, at


# ------------------------------------------------------------------------------------- 4: a culled repeat
def test_a_culled_frame_and_its_repeat(gpu, monkeypatch):
    """Second and third forward at one pose, from a scene pack: an occlusion-culled frame, then a GS_FRAME_CULL_REPEAT frame
    flagged by hand.  Images, cut tables and counters of default and GS_FWD_COMPACT=0 are equal, nothing fell back."""
    W, H = 64, 48
    scene, cam = _scene(W, H, 1), make_camera(W, H)
    got = {}
    for compact in (True, False):
        if compact:
            monkeypatch.delenv("GS_FWD_COMPACT", raising=False)
        else:
            monkeypatch.setenv("GS_FWD_COMPACT", "0")
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=MAX_PAIRS, auto_grow=False, force_strips=True, cull_second_pass="always")
        frames = []
        for k in range(2):
            r._cull_off_until = 0  # (the adaptive policy kept out of the way)
            image, _ = r.forward(*params, cam)
            st = r.stats()
            assert not st.cull_fallback and not st.cull_unrepaired and st.overflow == 0, (k, st)
            assert bool(r._frame.flags & CULL) == (k == 1) and r.scene_pack_active() == (k == 1)
            frames.append((image.clone(), r.cut_table().clone(), r.tile_compact_steps().clone(), (st.visible, st.pairs)))
        f, (image,) = _copy(r._frame, REPEAT)
        _lib.check(_lib.gs_frame_forward(C.byref(f), _stream()), "gs_frame_forward")
        visible, pairs, overflow, ran_past = _counters(f, 77)
        assert ran_past == 0 and overflow == 0
        frames.append((image, r.cut_table().clone(), r.tile_compact_steps().clone(), (visible, pairs)))
        got[compact] = frames
    for k, (a, b) in enumerate(zip(got[True], got[False])):
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and a[3] == b[3], k
        assert torch.equal(_bits(a[0]), _bits(got[True][0][0])), k  # the culled frames are the unculled one
        assert int((a[2] != -1).sum()) >= 8 and bool((b[2] == -1).all()), (k, a[2])
    assert got[True][1][3][1] < got[True][0][3][1]  # the culled frame emitted fewer pairs: its lists were trimmed


# ------------------------------------------------------------------------------------- 5: suspicious chunks
def test_suspicious_chunks_in_the_compact_phase(gpu, monkeypatch):
    """Background Gaussians with a NaN colour channel, an infinite scale and a zero scale, all deep in the lists: the tiles
    that list them have compacted by then, so their chunks take the compact loop's NaN-exact variant; and a zero scale in
    front, in a chunk of the full phase of tiles that compact later (the hand-over behind a suspicious chunk).  (The infinite scale
    gives an infinite covariance, which no tile lists -- in the oracle as on the device; it is in the scene for the stages in
    front.  The zero scale activates to 1e-4: a needle whose conic fails the chunk's test, and which IS listed.)"""
    W, H = 64, 48
    base = _scene(W, H, 1)
    scene = Scene(*(a.copy() for a in (base.pos, base.quat, base.scale, base.opa, base.rgb)))
    bg = 500 + np.argsort(-base.pos[500:2000, 2])[:40]  # the forty deepest background Gaussians
    centre = bg[np.argsort(np.abs(base.pos[bg, 0] / base.pos[bg, 2]) + np.abs(base.pos[bg, 1] / base.pos[bg, 2]))]
    nan_g, inf_g, needle_g = (int(g) for g in centre[:3])  # the three of them nearest to the middle of the frame
    scene.rgb[nan_g, 1] = np.nan
    scene.scale[inf_g, 0] = np.inf
    scene.scale[needle_g, 0] = 0.0
    # ... and a needle in FRONT: the nearest Gaussian of the opaque band around the middle of the frame.  Its chunk is a
    # suspicious one in the full phase, so the tiles that list it hand over with the vote refreshed through LDS.
    mid = np.nonzero((np.abs(base.pos[:500, 0] / base.pos[:500, 2]) < 0.2) & (np.abs(base.pos[:500, 1] / base.pos[:500, 2]) < 0.15))[0]
    early_g = int(mid[np.argmin(base.pos[mid, 2])])
    scene.scale[early_g, 0] = 0.0
    cam = make_camera(W, H)
    on = _run(gpu, monkeypatch, scene, cam, True)
    off = _run(gpu, monkeypatch, scene, cam, False)
    _same_everything(on, off)
    assert bool(torch.isnan(on["image"]).any())
    views = on["renderer"].debug_views()
    ranges, ids = views["tile_ranges"].cpu().numpy().reshape(-1, 2), views["sorted_ids"].cpu().numpy()
    at, cost = on["at"].cpu().numpy(), on["cost"].cpu().numpy()
    for g in (nan_g, needle_g):
        hit = []
        for t, (s, e) in enumerate(ranges):
            where = np.nonzero(ids[s:e] == g)[0]
            if len(where) and at[t] != -1 and at[t] <= where[0] < cost[t]:
                hit.append(t)
        print(f"Gaussian {g}: composited in the compact phase of tiles {hit}")
        assert hit, (g, at.tolist())
    before = [t for t, (s_, e_) in enumerate(ranges) if at[t] != -1 and (ids[s_:s_ + at[t]] == early_g).any()]
    print(f"Gaussian {early_g}: composited in the full phase of tiles {before}, which compacted afterwards")
    assert before, (early_g, at.tolist())


# ------------------------------------------------------------------------------------- 6: flagged long lists
def test_a_frame_flagged_for_long_lists_never_compacts(gpu, monkeypatch):
    W, H = 64, 48
    scene, cam = _scene(W, H, 2), make_camera(W, H)
    on = _run(gpu, monkeypatch, scene, cam, True, long_lists=True)
    off = _run(gpu, monkeypatch, scene, cam, False, long_lists=True)
    assert on["renderer"]._frame.flags & _lib.GS_FRAME_LONG_LISTS
    _same_everything(on, off)
    assert bool((on["at"] == -1).all()), on["at"]
    # (the same scene unflagged compacts in 9 of its 12 tiles: test_compact_equals_full_and_the_regimes_were_crossed)
