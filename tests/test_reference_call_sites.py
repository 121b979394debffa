"""CPU tier: every call the REFERENCE's own host files make into the two modules this package replaces -- `gaussian`
(the pybind11 extension, src/bindings.cpp:21-50) and `renderer` (renderer.py) -- binds to the replacement's signature.

The reference's Python cannot run here (CUDA-only device, third-party modules absent), so "renderer.py / splatter.py /
train.py work unchanged on top of this package"  is checked where it can be: the call sites
were taken from the reference's sources with `ast` -- number of positional arguments and keyword names of each
`gaussian.f(...)` / `renderer.f(...)` / `f(...)` imported from renderer -- and recorded in
tests/golden/reference_call_sites.json (tests/golden/make_golden.py::reference_call_sites), together with the attributes
its `_tocpp` methods store on the C++ objects; here they are bound against the shim's functions with
inspect.signature().bind().  What the calls COMPUTE is the business of the GPU parity tests
(tests/test_gpu_compat_pipeline.py drives the same sequence with real tensors)."""
import inspect
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_call_sites.json")


def recorded():
    with open(GOLD) as f:
        return json.load(f)


def test_every_reference_call_into_gaussian_and_renderer_binds_to_the_replacement():
    import gaussian
    import renderer

    targets = {"gaussian": gaussian, "renderer": renderer}
    seen = []
    for fname, line, mod, name, npos, kws in recorded()["calls"]:
        obj = getattr(targets[mod], name, None)
        assert obj is not None, f"{fname}:{line} calls {mod}.{name}, which the replacement does not have"
        if inspect.isclass(obj):  # gaussian.Tiles() / gaussian.Gaussian3ds(): default-constructible bags
            assert npos == 0 and not kws, f"{fname}:{line}"
            obj()
        else:
            sig = inspect.signature(obj)
            try:
                sig.bind(*([None] * npos), **{k: None for k in kws})
            except TypeError as e:
                raise AssertionError(f"{fname}:{line} {mod}.{name} with {npos} positional + {kws}: {e}") from e
        seen.append((fname, line, f"{mod}.{name}"))
    names = {s[2] for s in seen}
    # the call sites SURVEY.md section 8b lists (renderer.py:29,64,109,116,128,146; splatter.py:62,238,295,572,597 and
    # the renderer functions splatter.py imports)
    for must in ("gaussian.draw", "gaussian.draw_backward", "gaussian.world2camera", "gaussian.world2camera_backward",
                 "gaussian.global_culling", "gaussian.global_culling_backward", "gaussian.calc_tile_list",
                 "gaussian.gather_gaussians", "gaussian.jacobian", "gaussian.Tiles", "gaussian.Gaussian3ds",
                 "renderer.draw", "renderer.global_culling"):
        assert must in names, (must, sorted(names))


def test_attribute_bags_accept_what_the_reference_stores_in_them():
    """splatter.py:61-67 (Gaussian3ds._tocpp) and :295-300 (Tiles._tocpp) assign these attributes on the C++ objects."""
    import gaussian

    stored = recorded()["stored_attributes"]
    assert stored, "the reference's _tocpp assignments were not found"
    g, t = gaussian.Gaussian3ds(), gaussian.Tiles()
    for owner, attr in stored:
        assert hasattr(g if owner == "_cobj" else t, attr), (owner, attr)
