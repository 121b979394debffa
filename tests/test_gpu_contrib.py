"""GPU tier of the per-Gaussian contributions (csrc/contrib.hip through FrameRenderer.contributions; gs_prune_classify_contrib).

Scenes of 50 - 400 Gaussians on 64 x 48 and 70 x 45 images (the second has a padded border on both axes), built so that the
pair pass meets one tile with each of the list lengths 1, 63, 64, 65 and 130, a Gaussian whose 3 x 3 rectangle has an opaque
occluder over its middle tile (rows exist in some of its tiles and not in others), a footprint in the padded border only,
Gaussians behind the camera and one that covers the whole frame; N = 0 and N = 1; colour models 3 and 27, plain and aux frames,
an off-centre principal point, the "dist" listing method; two 160 x 120 frames (80 tiles) in which Gaussians have more than 64
rows each -- the frame-covering one under "prob2", nearly every one under "dist" with a listing radius of five tiles, whose
bounding squares have holes -- so that the Gaussian pass's wave-cooperative walk is held to the same checks; and a 32 x 32 frame with a pile of 2,100 faint Gaussians in one tile,
rendered as the renderer flags it and with GS_FRAME_LONG_LISTS forced.

Checks: (1) against the library's own backward, (2) against the float64 restatement (tests/contrib_ref.py) as an interval,
(3) per tile against the alpha map, (4) bitwise repeatability, accumulation, workspace independence, an overflowed frame,
(5) the backward is undisturbed, (6) gs_prune_classify_contrib against a torch mask.

Deviations measured on an MI355X are recorded in profiles/contrib_parity.txt."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from contrib_ref import composite, pixel_counts
from gaussian import _lib
from gs_frame import Contributions, FrameRenderer
from gs_prune import prune_options, prune_rows
from gs_scene import Scene, make_camera, make_scene
from gs_testutil import grad_close, to_torch

pytestmark = pytest.mark.gpu

W_MIN = 1.0 / 255.0
B = 1e-3  # the band of check 2: bounds the fp32 error of a transmittance product over the 2,100-entry list


# ----------------------------------------------------------------------------------------------------------- scenes
def _pad(v):
    return (v + 15) // 16 * 16


class _Builder:
    """Gaussians placed in PADDED pixel coordinates for make_camera(W, H): isotropic, identity rotation."""

    def __init__(self, W, H, seed):
        self.W, self.H, self.f = W, H, 0.75 * W
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def add(self, px, py, z, sigma_px, logit):
        x = (px - _pad(self.W) / 2) / self.f * z
        y = (py - _pad(self.H) / 2) / self.f * z
        s = max(sigma_px * abs(z) / self.f - 1e-4, 1e-6)
        self.rows.append((x, y, z, s, logit))
        return len(self.rows) - 1

    def scene(self):
        a = np.array(self.rows, np.float64).reshape(-1, 5)
        n = a.shape[0]
        quat = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
        return Scene(a[:, 0:3].astype(np.float32), quat.astype(np.float32), np.repeat(a[:, 3:4], 3, 1).astype(np.float32),
                     a[:, 4].astype(np.float32), self.rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32))


def _lists_scene():
    """64 x 48 (4 x 3 tiles, no border): five tiles with lists of 1, 63, 64, 65 and 130 small faint Gaussians."""
    b = _Builder(64, 48, 1)
    for (tx, ty), count in (((0, 0), 1), ((1, 0), 63), ((2, 0), 64), ((3, 0), 65), ((0, 2), 130)):
        for _ in range(count):
            b.add(16 * tx + 8 + b.rng.uniform(-3, 3), 16 * ty + 8 + b.rng.uniform(-3, 3), b.rng.uniform(1.0, 6.0), 1.3,
                  b.rng.uniform(-3.5, -2.0))
    return b.scene(), {}


def _occluder_scene(W, H):
    """70 opaque Gaussians over tile (1, 1) in front of one whose rectangle is 3 x 3 tiles around it: the middle tile stops
    inside its first bucket of 64, so the big Gaussian's pair there is never processed; a footprint in the padded border only
    (where there is one); five Gaussians behind the camera; one that covers the whole frame; small ones all over."""
    b = _Builder(W, H, 2)
    marks = {}
    for k in range(70):
        b.add(24.0, 24.0, 1.0 + 0.01 * k, 6.5, 8.0)  # 64 of them take T below 1e-4 within 13 pixels: the whole tile
    marks["big"] = b.add(24.0, 24.0, 5.0, 8.0, 1.0)
    if _pad(W) != W:
        marks["border"] = b.add(2.5, 20.5, 2.0, 0.12, 3.0)
    marks["behind"] = [b.add(b.rng.uniform(0, W), b.rng.uniform(0, H), -b.rng.uniform(0.5, 4.0), 3.0, 1.0) for _ in range(5)]
    marks["cover"] = b.add(_pad(W) / 2, _pad(H) / 2, 7.0, 150.0, -1.5)
    for _ in range(100):
        b.add(b.rng.uniform(0, _pad(W)), b.rng.uniform(0, _pad(H)), b.rng.uniform(0.6, 9.0), b.rng.uniform(0.8, 5.0),
              b.rng.normal(0.0, 2.0))
    return b.scene(), marks


def _pile_scene():
    """32 x 32: 2,100 faint Gaussians in tile (0, 0), a few elsewhere."""
    b = _Builder(32, 32, 3)
    for _ in range(2100):
        b.add(8 + b.rng.uniform(-2, 2), 8 + b.rng.uniform(-2, 2), b.rng.uniform(1.0, 8.0), 2.0, b.rng.uniform(-6.5, -5.5))
    for _ in range(20):
        b.add(b.rng.uniform(0, 32), b.rng.uniform(0, 32), b.rng.uniform(1.0, 8.0), 2.0, 0.0)
    return b.scene(), {}


def _random_scene(n, W, H, sh=False, seed=5):
    sc = make_scene(n, W, H, seed=seed, use_sh=sh)
    if not sh:
        sc.rgb = np.random.default_rng(seed).uniform(-2.0, 2.0, sc.rgb.shape).astype(np.float32)
    return sc, {}


def _wide_dist_scene():
    """160 x 120 for the "dist" listing method with a radius of five tiles: every Gaussian near the middle is listed in a disc
    cut out of the whole 10 x 8 grid -- up to 80 rows, with holes at the corners of its bounding square."""
    sc, _ = _random_scene(40, 160, 120, seed=13)
    return sc, {}


def _one_scene(W, H):
    b = _Builder(W, H, 4)
    b.add(_pad(W) / 2 + 3.0, _pad(H) / 2 - 2.0, 3.0, 4.0, 0.5)
    return b.scene(), {}


def _pp_camera(W, H):
    cam = make_camera(W, H, yaw_deg=1.0)
    cam.cx, cam.cy = W / 2 + 3.3, H / 2 - 2.6
    return cam


# name -> (scene builder, W, H, camera builder, forward kwargs, renderer kwargs)
CASES = {
    "lists": (_lists_scene, 64, 48, make_camera, {}, {}),
    "occluder64": (lambda: _occluder_scene(64, 48), 64, 48, make_camera, {}, {}),
    "occluder70_aux": (lambda: _occluder_scene(70, 45), 70, 45, make_camera, {"aux": True}, {}),
    "random70_sh27": (lambda: _random_scene(400, 70, 45, sh=True), 70, 45, make_camera, {}, {}),
    "random64_sh27_aux": (lambda: _random_scene(300, 64, 48, sh=True, seed=6), 64, 48, make_camera, {"aux": True}, {}),
    "random70_pp": (lambda: _random_scene(400, 70, 45, seed=7), 70, 45, _pp_camera, {}, {}),
    "random70_dist": (lambda: _random_scene(400, 70, 45, seed=8), 70, 45, make_camera, {},
                      {"tile_culling_method": "dist"}),
    "occluder160": (lambda: _occluder_scene(160, 120), 160, 120, make_camera, {}, {}),
    "wide160_dist": (_wide_dist_scene, 160, 120, make_camera, {}, {"tile_culling_method": "dist",
                                                                   "tile_culling_dist_thresh": 0.2}),
    "one": (lambda: _one_scene(70, 45), 70, 45, make_camera, {}, {}),
    "pile": (_pile_scene, 32, 32, make_camera, {}, {}),
    "pile_long_lists": (_pile_scene, 32, 32, make_camera, {}, {"long_lists": True}),
}
_CACHE = {}
DEVIATION = {}  # what check 2 measured: case -> (sum, max) largest distance outside [lo, hi] in units of t


def _case(gpu, name):
    """Renders the case as a training frame and evaluates the restatement at both ends of the band, once."""
    if name not in _CACHE:
        build, W, H, cam_fn, fkw, rkw = CASES[name]
        scene, marks = build()
        cam = cam_fn(W, H)
        params = to_torch(scene, gpu)
        r = FrameRenderer(gpu, max_pairs=1 << 16, training=True, **rkw)
        out = r.forward(*params, cam, training=True, **fkw)
        c = r.contributions(W_MIN)
        v = r.debug_views()
        f = r._frame
        args = (v["sorted_ids"].cpu(), v["tile_ranges"].cpu(), v["rec_geom"].cpu(), v["rec_cov"].cpu(), int(f.width),
                int(f.height), float(f.focal_x), float(f.focal_y))
        lo = composite(*args, stop=1e-4 * (1 + B), w_min=W_MIN * (1 + B))  # stops earlier, counts fewer
        hi = composite(*args, stop=1e-4 * (1 - B), w_min=W_MIN * (1 - B))
        _CACHE[name] = dict(scene=scene, marks=marks, cam=cam, params=params, r=r, out=out, c=c, rows=c.rows.clone(), lo=lo,
                            hi=hi, views=v, ids=args[0], ranges=args[1])
    return _CACHE[name]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------- 2. against the restatement
@pytest.mark.parametrize("name", list(CASES))
def test_contributions_lie_in_the_restatements_interval(gpu, name):
    k = _case(gpu, name)
    lo, hi, c = k["lo"], k["hi"], k["c"]
    n = k["scene"].n
    got_sum, got_max = c.weight_sum.cpu().double(), c.weight_max.cpu().double()
    got_pix, got_views = c.pixels.cpu().long(), c.views.cpu().long()
    t_lo = 1e-4 * lo.weight_sum.abs() + 1e-6 * lo.tile_pixels
    t_hi = 1e-4 * hi.weight_sum.abs() + 1e-6 * hi.tile_pixels
    out_sum = torch.maximum((lo.weight_sum - got_sum) / t_lo.clamp_min(1e-30), (got_sum - hi.weight_sum) / t_hi.clamp_min(1e-30))
    m_lo, m_hi = 1e-4 * lo.weight_max.abs() + 1e-6, 1e-4 * hi.weight_max.abs() + 1e-6
    out_max = torch.maximum((lo.weight_max - got_max) / m_lo, (got_max - hi.weight_max) / m_hi)
    DEVIATION[name] = (float(out_sum.max()) if n else 0.0, float(out_max.max()) if n else 0.0)
    pix_lo = pixel_counts(lo, n, k["ids"], W_MIN * (1 + B))
    pix_hi = pixel_counts(hi, n, k["ids"], W_MIN * (1 - B))
    lists = (k["ranges"][:, 1] - k["ranges"][:, 0]).tolist()
    print(f"contrib parity {name}: N {n} pairs {len(k['ids'])} longest list {max(lists)} | weight_sum: worst distance outside "
          f"[lo, hi] {DEVIATION[name][0]:+.3f} t | weight_max: {DEVIATION[name][1]:+.3f} t | pixels outside their interval: "
          f"{int(((got_pix < pix_lo) | (got_pix > pix_hi)).sum())} | interval width: sum {float((hi.weight_sum - lo.weight_sum).max()):.2e} "
          f"pixels {int((pix_hi - pix_lo).max())} | seen {int((got_views > 0).sum())}")
    assert bool((out_sum <= 1.0).all()), (name, int(out_sum.argmax()), float(out_sum.max()))
    assert bool((out_max <= 1.0).all()), (name, int(out_max.argmax()), float(out_max.max()))
    assert bool(((got_pix >= pix_lo) & (got_pix <= pix_hi)).all()), name
    assert torch.equal(got_views, (got_pix > 0).long())
    # what the scene was built for
    if name in ("occluder160", "wide160_dist"):  # more than 64 rows: the wave loads them, the owner still adds them in order
        touched = k["views"]["tiles_touched"].cpu()[k["views"]["visible"].cpu()]
        assert int(touched.max()) > 64 and int((touched > 64).sum()) >= (1 if name == "occluder160" else 10), touched.tolist()
        assert int(touched.min()) <= 64  # ... beside Gaussians of the same wave that take the per-lane walk
    if name == "lists":
        assert {1, 63, 64, 65, 130} <= set(lists), lists
    if name.startswith("pile"):
        assert max(lists) >= 2100
        assert bool(k["r"]._frame.flags & _lib.GS_FRAME_LONG_LISTS) == (name == "pile_long_lists")
    if name.startswith("occluder"):
        marks, touched = k["marks"], k["views"]["tiles_touched"].cpu()
        assert int(touched[marks["big"]]) == 9                      # a 3 x 3 rectangle ...
        assert k["r"].composited_steps() < len(k["ids"])             # ... and tiles that stopped inside their lists
        mid = 1 * (_pad(k["cam"].width) // 16) + 1
        assert lists[mid] > 64
        pos_in_mid = (k["ids"][k["ranges"][mid, 0]:k["ranges"][mid, 1]] == marks["big"]).nonzero()
        assert pos_in_mid.numel() == 1 and int(pos_in_mid) >= 64   # behind the first bucket: its row there does not exist
        assert float(got_sum[marks["big"]]) > 0.1                   # ... while those of its outer tiles do
        for g in marks["behind"]:
            assert not _bits(c.rows)[g].any()
        assert int(got_pix[marks["cover"]]) > 0
        if "border" in marks:
            assert int(touched[marks["border"]]) >= 1 and not _bits(c.rows)[marks["border"]].any()
    culled = ~k["views"]["visible"].cpu()
    assert not _bits(c.rows)[culled.numpy()].any()  # the row of a culled Gaussian is all zeros


def test_contributions_of_an_empty_scene(gpu):
    cam = make_camera(70, 45)
    empty = [torch.zeros(0, w, device=gpu) if w > 1 else torch.zeros(0, device=gpu) for w in (3, 4, 3, 1, 3)]
    r = FrameRenderer(gpu, max_pairs=1 << 12, training=True)
    r.forward(*empty, cam, training=True)
    c = r.contributions()
    assert tuple(c.rows.shape) == (0, 4) and c.pixels.numel() == 0
    out = Contributions.empty(0, gpu)
    assert r.contributions(out=out, accumulate=True) is out


# ------------------------------------------------------------------------------- 1. against the library's own backward
@pytest.mark.parametrize("name,bwd_rows", [("lists", False), ("lists", True), ("occluder64", False), ("occluder64", True),
                                           ("random70_pp", False), ("random70_dist", True), ("occluder160", False),
                                           ("wide160_dist", True)])
def test_weight_sum_is_the_colour_gradient_of_a_ones_image(gpu, name, bwd_rows):
    """dL/d(image)[..., 0] = 1: dL/d(rgb[g, 0]) = s (1 - s) sum_p w_g(p), s = sigmoid(rgb[g, 0]) -- the same fp32 stop
    decisions as the pass itself, so gs_testutil.grad_close's rule applies with the reference value as its own scale.  Raw
    colours lie in [-2, 2]: no pixel clamps, s (1 - s) >= 0.1."""
    build, W, H, cam_fn, fkw, rkw = CASES[name]
    scene, _ = build()
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 16, training=True, bwd_rows=bwd_rows, **rkw)
    image, _ = r.forward(*params, cam_fn(W, H), training=True)
    assert float(image.max()) < 1.0
    c = r.contributions()
    g = torch.zeros_like(image)
    g[..., 0] = 1.0
    grads = r.backward(g)
    assert bool(r._frame.flags & _lib.GS_FRAME_BWD_ROWS) == bwd_rows
    s = torch.sigmoid(params[4][:, 0].double())
    ref = (grads[4][:, 0].double() / (s * (1 - s))).cpu().numpy()
    ok, worst, where, pure = grad_close(c.weight_sum.cpu().numpy(), ref, np.abs(ref))
    print(f"contrib against the backward {name} rows={bwd_rows}: worst err / tol {worst:.3f}, within rtol alone {pure:.4f}")
    assert ok and float(np.abs(ref).max()) > 0.3, (name, worst, where)


# ------------------------------------------------------------------------------------------- 3. per tile, the alpha map
@pytest.mark.parametrize("name", ["occluder64", "occluder70_aux", "random70_dist", "random70_sh27", "wide160_dist"])
def test_pair_rows_add_up_to_the_alpha_map_per_tile(gpu, name):
    """The pair rows of a tile's list, read from the pass's workspace at the slots the gradient rows have (pair_offsets[g] + the
    tile's index in g's rectangle; the workspace zero-filled beforehand, so a row that does not exist reads 0), against the sum
    of render_aux's alpha map over the tile's image pixels: within 256 x 5e-5."""
    k = _case(gpu, name)
    r, cam = k["r"], k["cam"]
    _, _, _, alpha = FrameRenderer(gpu, max_pairs=1 << 16, **CASES[name][5]).forward(*k["params"], cam, training=False, aux=True)
    r._contrib_ws.zero_()
    r.forward(*k["params"], cam, training=True, **CASES[name][4])
    c = r.contributions()
    assert np.array_equal(_bits(c.rows), _bits(k["rows"]))  # (a zero-filled workspace: the same bytes)
    base = (r._contrib_ws.data_ptr() + 255) // 256 * 256 - r._contrib_ws.data_ptr() + 256
    pair = r._contrib_ws[base:base + 16 * int(r._frame.max_pairs)].view(torch.float32).reshape(-1, 4).cpu().double()
    rects = r._rects().cpu().long() & 0xffffffff
    vis = rects[:, 2] != 0
    touched = torch.where(vis, rects[:, 3], torch.zeros_like(rects[:, 3]))
    offs = torch.cumsum(touched, 0) - touched
    y0, x0, x1 = rects[:, 0] & 0xffff, rects[:, 1] & 0xffff, rects[:, 1] >> 16
    ntx = _pad(cam.width) // 16
    crop_top, crop_left = (_pad(cam.height) - cam.height) // 2, (_pad(cam.width) - cam.width) // 2
    padded = torch.zeros(_pad(cam.height), _pad(cam.width), dtype=torch.float64)
    padded[crop_top:crop_top + cam.height, crop_left:crop_left + cam.width] = alpha.cpu().double()
    worst = 0.0
    for t in range(k["ranges"].shape[0]):
        tx, ty = t % ntx, t // ntx
        g = k["ids"][k["ranges"][t, 0]:k["ranges"][t, 1]].long()
        slots = offs[g] + (ty - y0[g]) * (x1[g] - x0[g]) + (tx - x0[g])
        got = float(pair[slots, 0].sum())
        want = float(padded[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].sum())
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 256 * 5e-5, (name, t, got, want)
    print(f"contrib per tile {name}: worst |sum of pair rows - sum of alpha| {worst:.3e} over {k['ranges'].shape[0]} tiles")


# ------------------------------------------------------------------------------------------------------- 4. bitwise
def test_two_calls_and_any_workspace_bytes_give_the_same_rows(gpu):
    for name in ("occluder70_aux", "random70_sh27", "pile_long_lists", "lists", "occluder160", "wide160_dist"):
        k = _case(gpu, name)
        r = k["r"]
        r.forward(*k["params"], k["cam"], training=True, **CASES[name][4])
        again = r.contributions()
        assert np.array_equal(_bits(again.rows), _bits(k["rows"])), name
        for fill in (0x00, 0xFF):
            r._contrib_ws.fill_(fill)
            out = Contributions(torch.full((k["scene"].n * 16,), 0xFF, dtype=torch.uint8, device=gpu).view(torch.float32)
                                .view(-1, 4), W_MIN)
            assert np.array_equal(_bits(r.contributions(out=out).rows), _bits(k["rows"])), (name, fill)


def test_accumulate_over_three_views(gpu):
    scene, _ = _random_scene(400, 70, 45, seed=9)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=1 << 16, training=True)
    cams = [make_camera(70, 45, yaw_deg=y) for y in (-6.0, 0.0, 7.0)]
    singles = []
    acc = Contributions.empty(scene.n, gpu)
    for i, cam in enumerate(cams):
        r.forward(*params, cam, training=True)
        singles.append(r.contributions().rows.clone())
        r.contributions(out=acc, accumulate=True)
    s = [Contributions(t, W_MIN) for t in singles]
    want_sum = (s[0].weight_sum + s[1].weight_sum) + s[2].weight_sum  # the float sum in view order
    assert torch.equal(acc.weight_sum, want_sum)
    assert torch.equal(acc.weight_max, torch.maximum(torch.maximum(s[0].weight_max, s[1].weight_max), s[2].weight_max))
    assert torch.equal(acc.pixels, s[0].pixels + s[1].pixels + s[2].pixels)
    assert torch.equal(acc.views, s[0].views + s[1].views + s[2].views)
    assert int(acc.views.max()) == 3 and int(acc.views.min()) == 0 and not torch.equal(s[0].views, s[2].views)
    with pytest.raises(RuntimeError):
        r.contributions(accumulate=True)
    with pytest.raises(RuntimeError, match="w_min"):  # pixels / views counted at another floor do not add up
        r.contributions(0.5, out=acc, accumulate=True)
    with pytest.raises(RuntimeError):
        r.contributions(out=Contributions.empty(scene.n + 1, gpu))


def test_an_overflowed_frame_gives_zeros(gpu):
    scene, _ = _random_scene(400, 70, 45, seed=7)
    params = to_torch(scene, gpu)
    r = FrameRenderer(gpu, max_pairs=64, training=True, auto_grow=False)
    image, _ = r.forward(*params, make_camera(70, 45), training=True)
    out = Contributions(torch.full((scene.n * 16,), 0xFF, dtype=torch.uint8, device=gpu).view(torch.float32).view(-1, 4), W_MIN)
    r._contrib_ws = None
    c = r.contributions(out=out)
    assert r.stats().overflow > 64 and not image.any()
    assert not _bits(c.rows).any()


# --------------------------------------------------------------------------------------- 5. the backward is undisturbed
@pytest.mark.parametrize("what", ["rgb", "rgb_rows", "sh27", "aux"])
def test_backward_after_contributions_is_bitwise_the_backward(gpu, what):
    sh = what == "sh27"
    scene, _ = _random_scene(400, 70, 45, sh=sh, seed=10) if what != "rgb_rows" else _occluder_scene(70, 45)
    params = to_torch(scene, gpu)
    cam = make_camera(70, 45, yaw_deg=2.0)
    fkw = {"aux": True} if what == "aux" else {}
    rng = torch.Generator(device="cpu").manual_seed(3)
    g = torch.randn(45, 70, 3, generator=rng).to(gpu)
    bkw = {"grad_depth": torch.randn(45, 70, generator=rng).to(gpu), "grad_alpha": torch.randn(45, 70, generator=rng).to(gpu)} \
        if what == "aux" else {}
    results = []
    for with_call in (False, True, True):
        r = FrameRenderer(gpu, max_pairs=1 << 16, training=True, bwd_rows=(what == "rgb_rows"))
        r.forward(*params, cam, training=True, **fkw)
        if with_call:
            c = r.contributions()
            assert int(c.views.sum()) > 0
            if len(results) == 2:  # ... and once more, behind a stream synchronisation (the side stream has finished)
                torch.cuda.synchronize()
                r.contributions()
        results.append([_bits(t) for t in r.backward(g, **bkw)])
        if not with_call:  # behind a backward the preparation has been consumed: the pass builds the lists itself, the same
            c = r.contributions()
            for a, b in zip(results[0], [_bits(t) for t in r.backward(g, **bkw)]):
                assert np.array_equal(a, b), what
            first_rows = _bits(c.rows)
        elif len(results) == 2:
            assert np.array_equal(_bits(c.rows), first_rows), what
    for a, b, c2 in zip(*results):
        assert np.array_equal(a, b) and np.array_equal(a, c2), what
    assert any(a.any() for a in results[0])


# --------------------------------------------------------------------------------------- 6. gs_prune_classify_contrib
def test_classify_contrib_is_the_torch_mask(gpu):
    n = 4099
    g = np.random.default_rng(12)
    scale = torch.from_numpy(g.normal(0.0, 0.3, (n, 3)).astype(np.float32)).to(gpu)
    opa = torch.from_numpy(g.normal(0.0, 3.0, n).astype(np.float32)).to(gpu)
    rows = torch.zeros(n, 4, device=gpu)
    c = Contributions(rows, W_MIN)
    c.weight_sum.copy_(torch.from_numpy(g.uniform(0, 30, n).astype(np.float32)))
    c.weight_max.copy_(torch.from_numpy(g.uniform(0, 0.2, n).astype(np.float32)))
    c.pixels.copy_(torch.from_numpy(g.integers(0, 12, n).astype(np.int32)))
    c.views.copy_(torch.from_numpy(g.integers(0, 4, n).astype(np.int32)))
    c.weight_max[::50] = math.nan
    c.pixels[5::97] = -1  # a uint32 above 2^31: compared unsigned
    arrays = [scale, opa, rows, torch.from_numpy(g.normal(size=(n, 27)).astype(np.float32)).to(gpu)]
    base = (opa > float(np.float32(-math.log(1.0 / 0.02 - 1.0)))) & (scale.abs().square().sum(-1).sqrt() < 0.6)
    upix = c.pixels.long() & 0xffffffff
    for wmm, pm, vm in ((0.05, 3, 1), (0.0, 0, 1), (0.1, 0, 0), (0.0, 7, 3)):
        mask = base & (c.weight_max >= wmm) & (upix >= pm) & (c.views >= vm)  # (NaN >= x is False)
        out, kept, removed = prune_rows(scale, opa, arrays, opa_min=0.02, scale_max=0.6, contributions=c, weight_max_min=wmm,
                                        pixels_min=pm, views_min=vm)
        assert kept == int(mask.sum()) and kept + removed == n and 0 < kept < n, (wmm, pm, vm, kept)
        for o, a in zip(out, arrays):
            assert np.array_equal(_bits(o), _bits(a[mask]))  # (bits: the travelling contribution rows hold NaN)
    # copts = {0, 0, 0} reproduces gs_prune_classify's workspace bytes and counts (rows without NaN)
    clean = rows.clone()
    clean[::50, 1] = 0.0
    opts = prune_options(0.02, 0.6, "abs")
    res = []
    for contrib in (False, True):
        ws = torch.full((int(_lib.gs_prune_workspace_bytes(n)),), 0xFF, dtype=torch.uint8, device=gpu)
        counts = torch.full((2,), -1, dtype=torch.int64, device=gpu)
        stream = torch.cuda.current_stream().cuda_stream
        if contrib:
            co = _lib.GsPruneContribOpts(0.0, 0, 0)
            _lib.check(_lib.gs_prune_classify_contrib(scale.data_ptr(), opa.data_ptr(), clean.data_ptr(), n, C.byref(opts),
                                                      C.byref(co), counts.data_ptr(), ws.data_ptr(), ws.numel(), stream), "x")
        else:
            _lib.check(_lib.gs_prune_classify(scale.data_ptr(), opa.data_ptr(), n, C.byref(opts), counts.data_ptr(),
                                              ws.data_ptr(), ws.numel(), stream), "x")
        res.append((counts.tolist(), ws.cpu().numpy()))
    assert res[0][0] == res[1][0] == [int(base.sum()), n - int(base.sum())]
    assert np.array_equal(res[0][1], res[1][1])
