"""Generate tests/golden/*.npz from the REFERENCE itself (run in the build container only).

    python tests/golden/make_golden.py

Two sources, both the reference's own code executed here:
  A. its CUDA kernels (src/gaussian.cu) compiled for the CPU by oracle/build_ref.py and run on
     the SIMT emulator (oracle/ref.py)            -> kernels_*.npz
  B. its Python host code (splatter.Tiles, splatter.RayInfo, utils.q2r, utils.jacobian_torch,
     Gaussian3ds.get_gaussian_3d_cov, camera_to_image) imported from /root/reference with the
     missing third-party modules (kornia, cv2, pykdtree, the compiled `gaussian` extension)
     stubbed out -- none of them is touched by the functions used  -> host_geometry.npz

The fixtures are small (tens of KB) and committed; the tests that read them run anywhere.
Inputs are stored next to the outputs so that no generator state is needed to replay them.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]

import oracle  # noqa: E402
from gs_scene import make_camera, make_scene  # noqa: E402
from gs_testutil import OracleFrame, activate, frame_scalars  # noqa: E402
from oracle import build_ref, ref  # noqa: E402


def kernels_case(name, n, W, H, seed, use_sh, opa_shift, with_backward):
    scene = make_scene(n, W, H, seed=seed, use_sh=use_sh)
    scene.opa = (scene.opa + opa_shift).astype(np.float32)
    cam = make_camera(W, H, yaw_deg=2.0)
    cam.tran = np.array([0.04, -0.03, 0.15], np.float32)
    qn, sn = activate(scene)
    grid, hw, hh, rays = frame_scalars(cam)
    out = dict(pos=scene.pos, quat=qn, scale=sn, rot=cam.rot, tran=cam.tran, near=np.float32(cam.near),
               half_w=np.float32(hw), half_h=np.float32(hh), W=W, H=H, fx=np.float32(cam.focal_x),
               fy=np.float32(cam.focal_y), use_sh=use_sh)
    # K1 / K2
    rp, rc, mk = ref.global_culling(scene.pos, qn, sn, cam.rot, cam.tran, cam.near, hw, hh)
    rng = np.random.default_rng(seed + 100)
    gop = rng.normal(size=(n, 3)).astype(np.float32)
    goc = rng.normal(size=(n, 2, 2)).astype(np.float32)
    gp, gq, gs = ref.global_culling_backward(scene.pos, qn, sn, cam.rot, cam.tran, gop, goc, mk)
    out.update(k1_pos=rp, k1_cov=rc, k1_mask=mk, k2_gop=gop, k2_goc=goc, k2_gpos=gp, k2_gquat=gq, k2_gscale=gs)
    # K3 (three methods) / K6 on the culled set (splatter.py:536-541)
    keep = mk.astype(bool)
    pos_i, cov = rp[keep], rc[keep].reshape(-1, 4)
    maxp = max(len(pos_i) // 20, 8)  # splatter.py:569
    top, bottom, left, right = grid.tile_edges()
    geom = (grid.tile_geo_length_x, grid.tile_geo_length_y, grid.n_tile_x, grid.n_tile_y, grid.leftmost, grid.topmost)
    out.update(k3_maxp=maxp, k3_geom=np.array(geom, np.float64), tiles_top=top, tiles_bottom=bottom, tiles_left=left,
               tiles_right=right)
    for method in (0, 1, 2):
        thresh = 0.05 if method else (grid.tile_geo_length_x / 0.3) ** 2
        cnt, lst = ref.calc_tile_list(pos_i, cov, maxp, thresh, method, *geom, top, bottom, left, right)
        out[f"k3_m{method}_thresh"] = np.float32(thresh)
        out[f"k3_m{method}_count"] = cnt
        out[f"k3_m{method}_list"] = lst
        if method == 2:
            cntc = np.minimum(cnt, maxp)
            accum = np.concatenate([[0], np.cumsum(cntc)]).astype(np.int32)
            g, t = ref.gather_gaussians(accum, lst, int(cntc.max()))
            out.update(k6_accum=accum, k6_gathered=g, k6_tile_ids=t)
    # K7 / K8 on the canonically sorted pair list
    of = OracleFrame(scene, cam)
    kw = dict(use_sh=use_sh, fast=True, rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx, vdy=rays.dy)
    img = ref.draw(of.s_pos, of.s_rgb, of.s_opa, of.s_cov, of.accum, grid.padded_height, grid.padded_width,
                   grid.focal_x, grid.focal_y, **kw)
    out.update(k7_pos=of.s_pos, k7_rgb=of.s_rgb, k7_opa=of.s_opa, k7_cov=of.s_cov, k7_accum=of.accum, k7_image=img,
               rays_o=rays.rays_o, lefttop=rays.lefttop, vdx=rays.dx, vdy=rays.dy,
               max_per_tile=int(np.diff(of.accum).max()))
    if with_backward:
        gpad = rng.normal(size=img.shape).astype(np.float32)
        ref.reset_counters()
        g = ref.draw_backward(of.s_pos, of.s_rgb, of.s_opa, of.s_cov, of.accum, img, gpad, grid.focal_x, grid.focal_y,
                              **kw)
        out.update(k8_grad_output=gpad, k8_gpos=g[0], k8_grgb=g[1], k8_gopa=g[2], k8_gcov=g[3],
                   k8_undefined_reads=ref.undefined_reads())
    assert out["max_per_tile"] <= (340 if use_sh else 1200), "stay inside one forward chunk (see below)"
    np.savez_compressed(os.path.join(HERE, f"kernels_{name}.npz"), **out)
    print(name, "V", int(keep.sum()), "M", len(of.ids), "max/tile", out["max_per_tile"],
          "undefined shuffles", out.get("k8_undefined_reads"))


def host_geometry():
    """Reference Python host code with unavailable imports stubbed."""
    import torch

    class _Anything(types.ModuleType):
        def __getattr__(self, k):
            return type(k, (), {})

    for m in ("kornia", "cv2", "pykdtree", "pykdtree.kdtree", "gaussian"):
        sys.modules[m] = _Anything(m)
    sys.modules["kornia"].create_meshgrid = lambda *a, **k: None
    sys.modules["pykdtree.kdtree"].KDTree = object
    sys.path.insert(0, "/root/reference")
    for m in ("utils", "renderer", "splatter", "transforms"):
        sys.modules.pop(m, None)
    import splatter as ref_splatter  # the reference's splatter.py
    import utils as ref_utils  # the reference's utils.py

    out = {}
    cfgs = [(1920, 1080, 1440.0, 1440.0), (1297, 840, 961.3, 958.7), (256, 256, 192.0, 192.0), (333, 201, 250.5, 249.25)]
    for i, (W, H, fx, fy) in enumerate(cfgs):
        t = ref_splatter.Tiles(W, H, fx, fy, torch.device("cpu"))
        t.create_tiles()
        crop = t.crop(torch.arange(t.padded_height * t.padded_width * 3, dtype=torch.float32).reshape(
            t.padded_height, t.padded_width, 3))
        out[f"tiles{i}_cfg"] = np.array([W, H, fx, fy], np.float64)
        out[f"tiles{i}_scalars"] = np.array([t.padded_width, t.padded_height, t.n_tile_x, t.n_tile_y,
                                             t.tile_geo_length_x, t.tile_geo_length_y, t.leftmost, t.topmost],
                                            np.float64)
        out[f"tiles{i}_edges"] = np.stack([t.tiles_top.numpy(), t.tiles_bottom.numpy(), t.tiles_left.numpy(),
                                           t.tiles_right.numpy()])
        out[f"tiles{i}_crop_first"] = crop[0, 0].numpy()
        out[f"tiles{i}_crop_shape"] = np.array(crop.shape)
    rng = np.random.default_rng(77)
    q = rng.normal(size=(1, 4))
    rot = ref_utils.q2r(torch.from_numpy(q).float())[0]
    tran = torch.from_numpy(rng.normal(size=3)).float()
    ri = ref_splatter.RayInfo(rot, tran, 1088, 1920, 1440.0, 1437.5)
    out.update(ray_rot=rot.numpy(), ray_tran=tran.numpy(), ray_cfg=np.array([1088, 1920, 1440.0, 1437.5]),
               ray_o=ri.rays_o.numpy(), ray_lefttop=ri.lefttop.numpy(), ray_dx=ri.dx.numpy(), ray_dy=ri.dy.numpy())
    # projection through the reference's torch path (splatter.py:231-253 assembled from its own functions)
    n = 500
    pos = torch.from_numpy(rng.normal(size=(n, 3)) * [2, 2, 1] + [0, 0, 5]).float()
    quat = torch.from_numpy(rng.normal(size=(n, 4))).float()
    scale = torch.from_numpy(rng.normal(size=(n, 3)) * 0.05).float()
    g3 = ref_splatter.Gaussian3ds(pos=pos, rgb=torch.zeros(n, 3), opa=torch.zeros(n), quat=quat, scale=scale)
    cov3d = g3.get_gaussian_3d_cov(scale_activation="abs")
    pos_cam = pos @ rot.T + tran.unsqueeze(0)  # splatter.py:26 (the reference's torch world_to_camera)
    pos_img = ref_splatter.camera_to_image(pos_cam)
    J = ref_utils.jacobian_torch(pos_cam)
    JW = torch.matmul(J, rot.unsqueeze(0))
    cov2d = torch.bmm(torch.bmm(JW, cov3d), JW.permute(0, 2, 1))[:, :2, :2]
    out.update(proj_pos=pos.numpy(), proj_quat=quat.numpy(), proj_scale=scale.numpy(), proj_rot=rot.numpy(),
               proj_tran=tran.numpy(), proj_pos_cam=pos_cam.numpy(), proj_pos_img=pos_img.numpy(),
               proj_cov2d=cov2d.numpy(), proj_R=ref_utils.q2r(quat).numpy(), proj_J=J.numpy())
    np.savez_compressed(os.path.join(HERE, "host_geometry.npz"), **out)
    print("host_geometry ok")


def densify():
    """The reference's Gaussian3ds.adaptive_control (splatter.py:122-228) run as is on the CPU."""
    import torch

    class _Anything(types.ModuleType):
        def __getattr__(self, k):
            return type(k, (), {})

    for m in ("kornia", "cv2", "pykdtree", "pykdtree.kdtree", "gaussian"):
        sys.modules.setdefault(m, _Anything(m))
    sys.modules["kornia"].create_meshgrid = lambda *a, **k: None
    sys.modules["pykdtree.kdtree"].KDTree = object
    if "/root/reference" not in sys.path:
        sys.path.insert(0, "/root/reference")
    for m in ("utils", "renderer", "splatter", "transforms"):
        sys.modules.pop(m, None)
    import contextlib
    import io

    import splatter as ref_splatter

    out = {}
    cases = [("abs", "max", True, True), ("abs", "mean", False, True), ("exp", "max", True, True),
             ("abs", "max", True, False)]
    for ci, (act, agg, use_clone, use_split) in enumerate(cases):
        rng = np.random.default_rng(900 + ci)
        n = 600
        pos = rng.normal(size=(n, 3)).astype(np.float32) * 2
        quat = rng.normal(size=(n, 4)).astype(np.float32)
        scale = (rng.uniform(0.005, 0.12, size=(n, 3)) * rng.choice([-1, 1], size=(n, 3))).astype(np.float32)
        if act == "exp":
            scale = np.log(np.abs(scale)).astype(np.float32)
        opa = rng.normal(-2.0, 2.5, size=n).astype(np.float32)
        rgb = rng.normal(size=(n, 3)).astype(np.float32)
        grad = (rng.normal(size=(n, 3)) * 3e-4).astype(np.float32)
        g3 = ref_splatter.Gaussian3ds(*(torch.from_numpy(a.copy()) for a in (pos, rgb, opa)),
                                      quat=torch.from_numpy(quat.copy()), scale=torch.from_numpy(scale.copy()),
                                      init_values=True)
        seed = 4242 + ci
        torch.manual_seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            g3.adaptive_control(torch.from_numpy(grad.copy()), taus=0.05, delete_thresh=0.17, scale_activation=act,
                                grad_thresh=0.0002, grad_aggregation=agg, use_clone=use_clone, use_split=use_split,
                                clone_dt=0.01)
        # the normal draws MultivariateNormal.sample() consumed: two (n_split, 3) blocks from the same seed
        torch.manual_seed(seed)
        eps = [torch.normal(torch.zeros(n, 3), torch.ones(n, 3)) for _ in range(2)]  # upper bound on n_split rows
        out.update({f"c{ci}_cfg": np.array([act, agg, str(int(use_clone)), str(int(use_split))]),
                    f"c{ci}_seed": seed, f"c{ci}_pos": pos, f"c{ci}_quat": quat, f"c{ci}_scale": scale,
                    f"c{ci}_opa": opa, f"c{ci}_rgb": rgb, f"c{ci}_grad": grad,
                    f"c{ci}_out_pos": g3.pos.detach().numpy(), f"c{ci}_out_quat": g3.quat.detach().numpy(),
                    f"c{ci}_out_scale": g3.scale.detach().numpy(), f"c{ci}_out_opa": g3.opa.detach().numpy(),
                    f"c{ci}_out_rgb": g3.rgb.detach().numpy()})
        print("densify case", ci, act, agg, "N", n, "->", len(g3.pos))
    out["n_cases"] = len(cases)
    np.savez_compressed(os.path.join(HERE, "densify.npz"), **out)


def colmap():
    """Synthetic COLMAP binaries (written here, record layout of COLMAP's Reconstruction::Write*Binary) read back
    with the REFERENCE's readers (utils.py:111-141, 181-224, 259-294); files and parsed values are stored."""
    import struct

    import torch

    class _Anything(types.ModuleType):
        def __getattr__(self, k):
            return type(k, (), {})

    for m in ("kornia", "cv2", "pykdtree", "pykdtree.kdtree", "gaussian"):
        sys.modules.setdefault(m, _Anything(m))
    sys.modules["kornia"].create_meshgrid = lambda *a, **k: None
    if "/root/reference" not in sys.path:
        sys.path.insert(0, "/root/reference")
    for m in ("utils", "renderer", "splatter", "transforms"):
        sys.modules.pop(m, None)
    import utils as ref_utils

    d = os.path.join(HERE, "colmap")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(31)
    npar = {0: 3, 1: 4, 2: 4, 4: 8}
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        models = [1, 0, 2, 4]
        f.write(struct.pack("<Q", len(models)))
        for i, m in enumerate(models):
            f.write(struct.pack("<iiQQ", i + 1, m, 1920 + i, 1080 - i))
            f.write(struct.pack("<%dd" % npar[m], *rng.uniform(0.1, 2000, npar[m])))
    n_img, n_pts = 5, 300
    with open(os.path.join(d, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", n_img))
        for i in range(n_img):
            q = rng.normal(size=4)
            f.write(struct.pack("<i7di", 10 + i, *(q / np.linalg.norm(q)), *rng.normal(size=3), 1 + i % 4))
            f.write(("frame_%03d.JPG" % i).encode() + b"\x00")
            n2d = int(rng.integers(0, 40))
            f.write(struct.pack("<Q", n2d))
            for _ in range(n2d):
                f.write(struct.pack("<ddq", *rng.uniform(0, 1900, 2), int(rng.integers(-1, n_pts))))
    with open(os.path.join(d, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", n_pts))
        for i in range(n_pts):
            track = int(rng.integers(2, 7))
            f.write(struct.pack("<q3d3BdQ", 1000 + i, *rng.normal(size=3) * 3, *rng.integers(1, 255, 3).tolist(),
                                float(rng.uniform(0, 2)), track))
            f.write(struct.pack("<%di" % (2 * track), *rng.integers(0, 50, 2 * track).tolist()))
    cams = ref_utils.read_cameras_binary(os.path.join(d, "cameras.bin"))
    imgs = ref_utils.read_images_binary(os.path.join(d, "images.bin"))
    pts = ref_utils.read_points3d_binary(os.path.join(d, "points3D.bin"))
    out = {"cam_ids": np.array(sorted(cams)), "img_ids": np.array(sorted(imgs)), "pt_ids": np.array(list(pts))}
    for k, c in cams.items():
        out[f"cam{k}_model"] = np.array(c.model)
        out[f"cam{k}_wh"] = np.array([c.width, c.height])
        out[f"cam{k}_params"] = np.asarray(c.params)
    for k, im in imgs.items():
        out[f"img{k}_pose"] = np.concatenate([im.qvec, im.tvec])
        out[f"img{k}_cam"] = np.array(im.camera_id)
        out[f"img{k}_name"] = np.array(im.name)
        out[f"img{k}_xys"] = np.asarray(im.xys).reshape(-1, 2)
        out[f"img{k}_pids"] = np.asarray(im.point3D_ids)
        out[f"img{k}_rot"] = im.qvec2rotmat()
    out["pt_xyz"] = np.stack([p.xyz for p in pts.values()])
    out["pt_rgb"] = np.stack([p.rgb for p in pts.values()])
    out["pt_err"] = np.array([float(p.error) for p in pts.values()])
    out["pt_track_len"] = np.array([len(p.image_ids) for p in pts.values()])
    out["pt_image_ids"] = np.concatenate([p.image_ids for p in pts.values()])
    out["pt_p2d"] = np.concatenate([p.point2D_idxs for p in pts.values()])
    # the colour / SH initialisation of Splatter.__init__ (splatter.py:373-384) with the reference's helpers
    rgb = ref_utils.inverse_sigmoid_torch(torch.from_numpy(out["pt_rgb"] / 255.)).to(torch.float32)
    out["init_rgb"] = rgb.numpy()
    out["init_sh"] = ref_utils.initialize_sh(rgb).numpy()
    np.savez_compressed(os.path.join(HERE, "colmap.npz"), **out)
    print("colmap ok", len(cams), len(imgs), len(pts))


def train_cli():
    """Flags, types, defaults and choices of the reference's command line (train.py:296-363), read from its SOURCE
    with the ast module (importing train.py needs cv2 / torchmetrics / viser, which this image lacks)."""
    import ast
    import json

    src = open("/root/reference/train.py").read()
    out = {}
    for node in ast.walk(ast.parse(src)):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"):
            continue
        name = ast.literal_eval(node.args[0]).lstrip("-")
        kw = {k.arg: k.value for k in node.keywords}
        out[name] = {"type": kw["type"].id, "default": ast.literal_eval(kw["default"]),
                     "choices": ast.literal_eval(kw["choices"]) if "choices" in kw else None}
    json.dump(out, open(os.path.join(HERE, "train_cli.json"), "w"), indent=1, sort_keys=True)
    print("train_cli ok", len(out))


def reference_call_sites():
    """Every call of the reference's host files into `gaussian` / `renderer` (function, number of positional arguments,
    keyword names, line) and the attributes splatter.py's _tocpp methods store on the C++ objects, read from its SOURCE
    with the ast module -> reference_call_sites.json (tests/test_reference_call_sites.py binds them to this package)."""
    import ast
    import json

    ref_root = os.path.dirname(os.path.dirname(build_ref.REF_SRC))

    def module_calls(path, module_names, imported_from):
        tree = ast.parse(open(path).read(), filename=path)
        direct = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module in imported_from:
                direct.update(a.asname or a.name for a in node.names)
        out = []
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            fn = node.func
            name = mod = None
            if isinstance(fn, ast.Attribute) and isinstance(fn.value, ast.Name) and fn.value.id in module_names:
                mod, name = fn.value.id, fn.attr
            elif isinstance(fn, ast.Name) and fn.id in direct:
                mod, name = next(iter(imported_from)), fn.id
            if name is None or any(isinstance(a, ast.Starred) for a in node.args) or any(k.arg is None for k in node.keywords):
                continue
            out.append((mod, name, len(node.args), [k.arg for k in node.keywords], node.lineno))
        return out

    calls = []
    for fname in ("renderer.py", "splatter.py", "train.py", "visergui.py"):
        path = os.path.join(ref_root, fname)
        if os.path.exists(path):
            calls += [[fname, line, mod, name, npos, kws]
                      for mod, name, npos, kws, line in module_calls(path, {"gaussian", "renderer"}, {"renderer"})]
    stored = set()
    for node in ast.walk(ast.parse(open(os.path.join(ref_root, "splatter.py")).read())):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id in ("_cobj", "_tile"):
                    stored.add((t.value.id, t.attr))
    with open(os.path.join(HERE, "reference_call_sites.json"), "w") as f:
        json.dump({"calls": calls, "stored_attributes": sorted(list(x) for x in stored)}, f, indent=1)
    print("reference_call_sites ok", len(calls), len(stored))


def ref_live():
    """The reference kernels' outputs on the inputs of tests/test_ref_live.py -> ref_live.npz: the module's tests run
    once with the live library, recording what they receive from it."""
    import test_ref_live

    test_ref_live.RECORD = {}
    for seed in (31, 32):
        test_ref_live.test_oracle_vs_reference_kernels_fresh_seed(seed)
    test_ref_live.test_reference_backward_defect_between_chunks_is_real()
    for use_sh in (False, True):
        test_ref_live.test_sigmoid_flag_forward_and_backward_vs_reference_kernels(use_sh)
    for use_sh in (False, True):
        test_ref_live.test_oracle_vs_reference_kernels_general_camera(use_sh)
    np.savez_compressed(os.path.join(HERE, "ref_live.npz"), **test_ref_live.RECORD)
    print("ref_live ok", len(test_ref_live.RECORD))


if __name__ == "__main__":
    assert os.path.isdir("/root/reference"), "needs the reference checkout"
    oracle.build()
    build_ref.build()
    kernels_case("nosh", 700, 64, 48, seed=21, use_sh=False, opa_shift=-3.0, with_backward=True)
    kernels_case("sh", 330, 48, 32, seed=6, use_sh=True, opa_shift=-3.0, with_backward=True)
    # <= 1200 Gaussians per tile: beyond one shared-memory chunk the reference forward kernel has a
    # race (no barrier after its compute loop, gaussian.cu:878-962) that the emulator's serial
    # schedule exposes deterministically (measured: 5 tiles of 1450 -> max image error 0.47).
    kernels_case("dense_fwd", 4500, 64, 48, seed=22, use_sh=False, opa_shift=1.5, with_backward=False)
    host_geometry()
    densify()
    colmap()
    train_cli()
    reference_call_sites()
    ref_live()
