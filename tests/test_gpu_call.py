"""Every door of the Python layer refuses a tensor that is not a contiguous float32 HIP tensor (of the door's shape, where it
has one) by the argument's name, before anything is launched."""
import numpy as np
import pytest
import torch

import gs_densify
import gs_prune
import gs_seed
from gs_icp import IcpAligner
from gs_pyramid import Pyramid
from gs_scene import make_camera
from gs_slam import view_overlap
from gs_track import Tracker
from gs_train import DepthLoss, GatedTrackLoss, ImageLoss, TrackLoss

S, N = 8, 8  # the maps are S x S, a Gaussian set holds N rows
FIVE = ("pos", "quat", "scale", "opa", "rgb")


def _bad(good: torch.Tensor, fixed: bool):
    """The bad versions of a good argument: float64; a non-contiguous view of the same shape (transposed; a vector: a column
    of a matrix); and, where the door fixes the shape, a good tensor with one dimension more."""
    shape = tuple(good.shape)
    yield good.double()
    if good.dim() == 1:
        yield good.new_zeros(shape[0], 2)[:, 0]
    else:
        yield good.new_zeros(shape[::-1]).permute(*reversed(range(good.dim())))
    if fixed:
        yield good.new_zeros(shape + (2,))


@pytest.mark.gpu
def test_every_door_names_the_tensor_it_refuses(gpu):
    def z(*shape):
        return torch.zeros(*shape, dtype=torch.float32, device=gpu)

    cam = make_camera(S, S)
    maps = lambda *names: {k: z(S, S, 3) if "image" in k or k == "pred" else z(S, S) for k in names}  # noqa: E731
    gaussians = {"pos": z(N, 3), "quat": z(N, 4), "scale": z(N, 3), "opa": z(N), "rgb": z(N, 3)}
    sopts, popts = gs_seed.seed_options(), gs_prune.prune_options()
    pyramid = Pyramid(S, S, 1, gpu)
    losses = {cls.__name__: cls(S, S, device=gpu) for cls in (ImageLoss, DepthLoss, TrackLoss, GatedTrackLoss)}
    tracker = Tracker(list(gaussians.values()), cam, None, gpu)
    icp = IcpAligner(cam, None, gpu)
    icp.set_model(z(S, S), z(S, S), np.eye(3), np.zeros(3))  # (align needs a model: the test's one launch)
    track_maps = maps("image", "depth", "alpha", "target_image", "target_range")
    # (door, its call on a dict of arguments by name, the good arguments, does the door fix their shapes?)
    doors = [
        ("seed_classify", lambda a: gs_seed.seed_classify(a["depth"], None, sopts), maps("depth"), False),
        ("seed_classify", lambda a: gs_seed.seed_classify(z(S, S), (a["rendered depth"], a["rendered alpha"]), sopts),
         maps("rendered depth", "rendered alpha"), True),
        ("seed_apply", lambda a: gs_seed.seed_apply(a["image"], z(S, S), cam, sopts, [a[k] for k in FIVE], 0, None, None),
         {**maps("image"), **gaussians}, True),
        ("Pyramid.build", lambda a: pyramid.build(a["image"], a["range_map"]), maps("image", "range_map"), True),
        ("ImageLoss", lambda a: losses["ImageLoss"](a["pred"], a["target"]),
         {"pred": z(S, S, 3), "target": z(S, S, 3)}, True),
        ("DepthLoss", lambda a: losses["DepthLoss"](a["depth"], a["alpha"], a["target"], 1.0),
         maps("depth", "alpha", "target"), True),
        ("TrackLoss", lambda a: losses["TrackLoss"](*(a[k] for k in track_maps), 1.0), track_maps, True),
        ("GatedTrackLoss", lambda a: losses["GatedTrackLoss"](*(a[k] for k in track_maps), 1.0), track_maps, True),
        ("view_overlap", lambda a: view_overlap(a["range_map"], cam, a["table"], 4, table_pp=a["table_pp"]),
         {"range_map": z(S, S), "table": z(4, 16), "table_pp": z(4, 2)}, True),
        ("prune_classify", lambda a: gs_prune.prune_classify(a["scale"], a["opa"], popts),
         {"scale": z(N, 3), "opa": z(N)}, False),
        ("adaptive_control", lambda a: gs_densify.adaptive_control([a[k] for k in FIVE], a["grad"], 0.05, 1.5),
         {**gaussians, "grad": z(N, 3)}, True),
        ("Tracker.set_map", lambda a: tracker.set_map([a[k] for k in FIVE]), gaussians, False),
        ("IcpAligner.set_model", lambda a: icp.set_model(a["depth"], a["alpha"], np.eye(3), np.zeros(3)),
         maps("depth", "alpha"), True),
        ("IcpAligner.align", lambda a: icp.align(a["range_map"]), maps("range_map"), True),
    ]
    table = [(door, call, good, name, bad) for door, call, good, fixed in doors for name, t in good.items()
             for bad in _bad(t, fixed)]
    assert len(table) == sum((3 if fixed else 2) * len(good) for _, _, good, fixed in doors) > 100
    for door, call, good, name, bad in table:
        with pytest.raises(RuntimeError, match=f"^{name} must be a contiguous float32 HIP tensor"):
            call({**good, name: bad})
            pytest.fail(f"{door} took {name} as float64 / strided / misshapen: {bad.dtype}, {tuple(bad.shape)}, {bad.stride()}")
