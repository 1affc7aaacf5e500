"""The NeuS render composite (nr3d_neus_composite_fwd / _bwd, graphics.neus.neus_render) -- what can be checked without a GPU: the ABI,
the binding's argument counts, the module's surface, and the op-chain route of ``composite_volume_buffer`` on CPU tensors against the
float64 evaluation of the restated reference chain (tests/neus_render_ref.py)."""
import ast
import inspect
import os

import pytest
import torch

import neus_render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_and_symbols():
    from nr3d_lib_amd import _abi
    assert _abi.ABI_VERSION >= 25
    fwd, bwd = _abi.SIGNATURES["nr3d_neus_composite_fwd"], _abi.SIGNATURES["nr3d_neus_composite_bwd"]
    assert fwd[0] == bwd[0] == "int"
    assert fwd[1] == ["int", "uint32_t", "uint64_t", "uint32_t"] + ["ptr"] * 6 + ["float", "float", "int", "int"] + ["ptr"] * 6
    assert bwd[1] == ["int", "uint32_t", "uint64_t", "uint32_t"] + ["ptr"] * 6 + ["float", "float", "int", "int"] + ["ptr"] * 13


def test_binding_argument_counts():
    """every call of the two entry points in the binding passes as many arguments as the header declares: head() holds the shared 14"""
    from nr3d_lib_amd import _abi
    from nr3d_lib_amd.bindings import _neus_composite as b
    tree = ast.parse(inspect.getsource(b))
    head = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "head")
    ret = next(n for n in ast.walk(head) if isinstance(n, ast.Return)).value
    n_head = sum(1 for e in ret.elts if not isinstance(e, ast.Starred)) + 4         # *self.tail: eps, thre, normalize, normals_mode
    assert n_head == 14
    seen = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("nr3d_neus_composite_"):
            assert isinstance(node.args[0], ast.Starred)
            seen[node.func.attr] = n_head + len(node.args) - 1
    assert seen == {name: len(_abi.SIGNATURES[name][1]) for name in ("nr3d_neus_composite_fwd", "nr3d_neus_composite_bwd")}


def test_surface():
    from nr3d_lib_amd.graphics import neus
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    assert nr.__all__ == ['NeusComposite', 'ray_composite', 'packed_composite_normals', 'composite_volume_buffer']
    assert all(getattr(neus, name) is getattr(nr, name) for name in nr.__all__)
    assert isinstance(nr.FUSED_NEUS_COMPOSITE, bool)
    assert list(inspect.signature(nr.ray_composite).parameters) == ["alpha", "t", "rgb", "nablas", "rays_inds_hit", "num_rays",
                                                                    "normalize_depth", "normalized_normals"]
    assert list(inspect.signature(nr.packed_composite_normals).parameters)[:5] == ["alpha", "t", "rgb", "nablas", "pack_infos"]
    assert list(inspect.signature(nr.composite_volume_buffer).parameters) == ["volume_buffer", "num_rays", "with_rgb", "with_normal",
                                                                              "training", "depth_use_normalized_vw", "device", "dtype"]


def _buffer(inp):
    t = lambda a: None if a is None else torch.from_numpy(a).clone()        # noqa: E731
    buf = dict(type="batched" if inp["layout"] == "rows" else "packed", opacity_alpha=t(inp["alpha"]), t=t(inp["t"]), rgb=t(inp["rgb"]),
               nablas=t(inp["nablas"]), rays_inds_hit=t(inp["rays_inds_hit"]))
    if inp["pack_infos"] is not None:
        buf["pack_infos_hit"] = t(inp["pack_infos"])
    return buf


def _close(name, got, want64):
    scale = float(want64.abs().max()) or 1.0
    err = float((got.double() - want64).abs().max()) / scale
    assert err <= 1e-5, f"{name}: rel err {err:.2e}"


@pytest.mark.parametrize("inp", [ref.rows_inputs(5, 7), ref.rows_inputs(3, 65, kind="opaque"), ref.rows_inputs(3, 1), ref.pack_inputs(13)],
                         ids=["rows5x7", "rows3x65opaque", "rows3x1", "packs13"])
@pytest.mark.parametrize("training", [True, False])
def test_volume_buffer_chain_on_cpu(inp, training):
    """CPU tensors take the op chain; 1e-5 of the output's maximum is fp32 rounding of sums of at most 200 terms of one sign pattern
    (the same floor as the GPU yardstick)"""
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    buf = _buffer(inp)
    out = nr.composite_volume_buffer(buf, inp["num_rays"], training=training, depth_use_normalized_vw=True)
    want = ref.evaluate(inp, torch.float64, "cpu", normalized_normals=not training, grads=False)
    _close("vw", buf["vw"], want["vw"])
    for k, name in (("mask", "mask_volume"), ("depth", "depth_volume"), ("rgb", "rgb_volume"), ("normals", "normals_volume")):
        assert out[name].shape == want[k].shape
        _close(name, out[name], want[k])
    clamped = torch.from_numpy(inp["nablas"]).clamp(-1, 1)
    assert torch.equal(buf["nablas"], torch.from_numpy(inp["nablas"]) if training else clamped)     # evaluation clamps in place
    few = nr.composite_volume_buffer(_buffer(inp), inp["num_rays"], with_rgb=False, with_normal=False, depth_use_normalized_vw=False)
    assert sorted(few) == ["depth_volume", "mask_volume"]
    _close("depth_volume", few["depth_volume"], ref.evaluate(inp, torch.float64, "cpu", normalize_depth=False, grads=False)["depth"])


def test_volume_buffer_empty():
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    out = nr.composite_volume_buffer(dict(type="empty"), 6, device="cpu")
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(mask_volume=(6,), depth_volume=(6,), rgb_volume=(6, 3), normals_volume=(6, 3))
    assert all(not v.any() and v.dtype == torch.float32 for v in out.values())
    assert sorted(nr.composite_volume_buffer(dict(type="empty"), 2, with_rgb=False, with_normal=False)) == ["depth_volume", "mask_volume"]
    with pytest.raises(RuntimeError, match="unknown volume buffer type"):
        nr.composite_volume_buffer(dict(type="octree"), 2)


def test_chain_gradients_on_cpu():
    """the op chain is differentiable on CPU tensors in both layouts and gives the float64 gradients"""
    from nr3d_lib_amd.graphics.neus import neus_render as nr
    for inp in (ref.rows_inputs(4, 9), ref.pack_inputs(7)):
        want = ref.evaluate(inp, torch.float64, "cpu")
        leaf = lambda a: torch.from_numpy(a).clone().requires_grad_(True)       # noqa: E731
        alpha, t, rgb, nablas = leaf(inp["alpha"]), leaf(inp["t"]), leaf(inp["rgb"]), leaf(inp["nablas"])
        hit = torch.from_numpy(inp["rays_inds_hit"])
        if inp["layout"] == "rows":
            out = nr.ray_composite(alpha, t, rgb, nablas, hit, inp["num_rays"])
        else:
            out = nr.packed_composite_normals(alpha, t, rgb, nablas, torch.from_numpy(inp["pack_infos"]), hit, inp["num_rays"])
        cot = ref.cotangents(inp)
        loss = sum((o * torch.from_numpy(cot[k])).sum() for k, o in zip(ref.OUTPUTS, out))
        for k, g in zip(ref.GRADS, torch.autograd.grad(loss, [alpha, t, rgb, nablas])):
            _close(k, g, want[k])


def test_routes(monkeypatch):
    """the fused route needs the switch, GPU float32 tensors and no gradient through normalised normals; everything else is the chain"""
    from nr3d_lib_amd.graphics.neus import neus_render as nr

    class Fake:
        """a stand-in with the properties the route looks at"""
        def __init__(self, is_cuda=True, dtype=torch.float32, requires_grad=False):
            self.is_cuda, self.dtype, self.requires_grad = is_cuda, dtype, requires_grad

    a, g = Fake(), Fake(requires_grad=True)
    monkeypatch.setattr(nr, "FUSED_NEUS_COMPOSITE", True)
    assert nr._fused(a, a, a, a, False) and nr._fused(a, a, None, None, False) and nr._fused(g, a, a, g, False)
    assert nr._fused(a, a, a, a, True)                          # evaluation without gradients: the kernel clamps and normalises
    assert not nr._fused(a, a, a, g, True) and not nr._fused(g, a, a, a, True)      # no backward for that form
    with torch.no_grad():
        assert nr._fused(a, a, a, g, True)
    assert nr._fused(g, a, a, None, True)                       # no nablas, nothing to normalise
    assert not nr._fused(Fake(is_cuda=False), a, a, a, False) and not nr._fused(a, a, Fake(dtype=torch.float64), a, False)
    monkeypatch.setattr(nr, "FUSED_NEUS_COMPOSITE", False)
    assert not nr._fused(a, a, a, a, False)
