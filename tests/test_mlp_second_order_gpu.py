"""GPU: the fused double backward of the fp32 decoder (csrc/mlp.hip k_mlp_bwd2 through bindings._mlp.backward_backward and
models.blocks.mlp.FusedMLPBackwardFunction) -- the eikonal term of an SDF step -- against torch's own double backward.

Yardstick as tests/test_mlp_gpu.py: the error against a float64 evaluation stays within a few times torch's own fp32 error."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# dims, n, hidden act, out act, bias: the backward-fusable CASES of test_mlp_gpu.py, the LoTD-NeuS decoder, and the variants
CASES = [
    ([32, 32, 16], 4099, "relu", None, True),
    ([32, 64, 64, 16], 10007, "relu", None, True),
    ([18, 64, 3], 777, "relu", "relu", True),
    ([16, 32, 32, 32, 7], 4097, "relu", None, False),
    ([40, 48, 33], 33, None, None, True),
    ([3, 8, 1], 1, "relu", None, True),
    ([64, 64, 64], 2048, "relu", None, True),
    ([35, 64, 1], 3001, "relu", None, True),
    ([32, 64, 64, 1], 1000, "relu", None, True),
    ([64, 64, 64, 64], 513, "relu", None, True),
]


def _net(dims, hidden, out, bias, dev, seed=0, dtype=torch.float):
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(seed)
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=hidden or "none", output_activation=out, bias=bias,
            dtype=dtype, device=dev)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.4 if p.dim() > 1 else 0.2))
    return m


def _desc(m):
    from nr3d_lib_amd.bindings import _mlp
    return _mlp.MLPDesc([m.in_features, *m.Ws, m.out_features], m._act_code(m.layers[0]), m._act_code(m.layers[-1]))


def _params(m):
    return [l.weight for l in m.layers], [l.bias for l in m.layers]


def _double_reference(m, x, gy, v, dtype):
    """torch's double backward in `dtype`: d <dL/dx, v> / d(W_l, dL_dy) with dL/dx = autograd of the layer-by-layer network"""
    xd = x.detach().to(dtype)
    ws = [l.weight.detach().to(dtype).requires_grad_(True) for l in m.layers]
    bs = [None if l.bias is None else l.bias.detach().to(dtype) for l in m.layers]
    g = gy.detach().to(dtype).requires_grad_(True)
    xi = xd.clone().requires_grad_(True)
    h = xi
    for l, W, b in zip(m.layers, ws, bs):
        h = torch.nn.functional.linear(h, W, b)
        if l.activation is not None:
            h = torch.relu(h)
    dx, = torch.autograd.grad(h, xi, g, create_graph=True)
    got = torch.autograd.grad((dx * v.detach().to(dtype)).sum(), [*ws, g], allow_unused=True)
    return [w if w is not None else torch.zeros_like(W) for w, W in zip(got[:-1], ws)], got[-1]


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64).abs().max()) / scale
    err32 = float((ref32.double() - ref64).abs().max()) / scale
    assert err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 path: {err32:.2e})"


def _layouts(t, layout):
    """[n, w] -> the same values in `layout`: row-major, feature-major ([w, n] storage) or rows with a padded stride"""
    if layout == "feature_major":
        return t.t().contiguous().t()
    if layout == "strided":
        n, w = t.shape
        buf = torch.full((n, w + 5), float("nan"), device=t.device)
        buf[:, :w] = t
        return buf[:, :w]
    return t.contiguous()


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("dims,n,hidden,out,bias", CASES)
def test_binding_matches_torch_double_backward(dev, hip_option, x3, dims, n, hidden, out, bias):
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    m = _net(dims, hidden, out, bias, dev)
    d = _desc(m)
    assert d.second_order_fusable
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(n, dims[0], generator=g).to(dev)
    gy = torch.randn(n, dims[-1], generator=g).to(dev)
    v = torch.randn(n, dims[0], generator=g).to(dev)
    ws, bs = _params(m)
    packed = _mlp.pack(d, ws, bs, with_backward=True)
    ref64, ggy64 = _double_reference(m, x, gy, v, torch.float64)
    ref32, ggy32 = _double_reference(m, x, gy, v, torch.float32)
    for layout in ("row", "feature_major", "strided"):
        dgy, dWs, dbs = _mlp.backward_backward(d, _layouts(x, layout), gy, _layouts(v, layout), packed, need_dgy=True)
        assert dbs == [None] * len(ws)
        assert torch.isfinite(dgy).all(), f"{layout}: dL/d(dL_dy) not fully written"
        _check(f"{layout} dL/d(dL_dy)", dgy, ggy64, ggy32)
        for l, (a, r64, r32) in enumerate(zip(dWs, ref64, ref32)):
            _check(f"{layout} dW[{l}]", a, r64, r32)
    # no dL/d(dL_dy) wanted; zero bias views asked for
    dgy, dWs2, dbs = _mlp.backward_backward(d, x, gy, v, packed, need_dgy=False, has_bias=[True] * len(ws))
    assert dgy is None and all(b is not None and not b.any() for b in dbs)
    for l, (a, r64, r32) in enumerate(zip(dWs2, ref64, ref32)):      # (atomics: the summation order differs between runs)
        _check(f"need_dgy=False dW[{l}]", a, r64, r32)


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("dims,out", [([35, 64, 1], None), ([32, 64, 64, 16], "relu")])
def test_binding_stride0_dL_dy_and_odd_n(dev, hip_option, x3, dims, out):
    """dL_dy as an expanded ones (row stride 0, what autograd hands the sdf column) and n = 1, 33, 100 (not a multiple of 32)"""
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    m = _net(dims, "relu", out, True, dev, seed=3)
    d = _desc(m)
    ws, bs = _params(m)
    packed = _mlp.pack(d, ws, bs, with_backward=True)
    g = torch.Generator(device="cpu").manual_seed(2)
    for n in (1, 33, 100):
        x = torch.randn(n, dims[0], generator=g).to(dev)
        v = torch.randn(n, dims[0], generator=g).to(dev)
        gy = torch.ones(1, 1, device=dev).expand(n, dims[-1])
        ref64, ggy64 = _double_reference(m, x, gy, v, torch.float64)
        ref32, ggy32 = _double_reference(m, x, gy, v, torch.float32)
        dgy, dWs, _ = _mlp.backward_backward(d, x, gy, v, packed, need_dgy=True)
        assert tuple(dgy.shape) == (n, dims[-1]) and torch.isfinite(dgy).all()
        _check(f"n={n} dL/d(dL_dy)", dgy, ggy64, ggy32)
        for l, (a, r64, r32) in enumerate(zip(dWs, ref64, ref32)):
            _check(f"n={n} dW[{l}]", a, r64, r32)


def test_create_graph_routes_through_the_fused_double_backward(dev):
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net([35, 64, 1], "relu", None, True, dev, seed=1)
    x = torch.randn(1000, 35, device=dev, requires_grad=True)
    nablas, = torch.autograd.grad(m(x)[:, 0].sum(), x, create_graph=True)
    assert type(nablas.grad_fn).__name__ == "FusedMLPBackwardFunctionBackward"
    d = m.fused_desc()
    ws, bs = _params(m)
    dx, _, _ = _mlp.backward(d, x.detach(), torch.ones(1000, 1, device=dev), _mlp.pack(d, ws, bs, with_backward=True))
    assert torch.equal(nablas, dx)
    mlp_mod.FUSED_SECOND_ORDER = False
    try:
        nablas_t, = torch.autograd.grad(m(x)[:, 0].sum(), x, create_graph=True)
    finally:
        mlp_mod.FUSED_SECOND_ORDER = True
    assert type(nablas_t.grad_fn).__name__ != "FusedMLPBackwardFunctionBackward"
    torch.testing.assert_close(nablas_t, nablas, rtol=1e-4, atol=1e-5)


def _eikonal_step(m, x0, dt=torch.float32):
    m.zero_grad(set_to_none=True)
    x = x0.to(dt).clone().requires_grad_(True)
    y = m(x)
    nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
    loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + y.square().mean()
    loss.backward()
    return [p.grad.clone() for p in m.parameters()], x.grad.clone()


@pytest.mark.parametrize("dims,out", [([35, 64, 1], None), ([32, 64, 64, 16], None), ([18, 64, 3], "relu"), ([32, 32, 32, 32, 4], None)])
def test_eikonal_step_matches_torch_and_float64(dev, dims, out):
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net(dims, "relu", out, True, dev, seed=7)
    x0 = torch.randn(3000, dims[0], generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    gf, xf = _eikonal_step(m, x0)
    mlp_mod.USE_FUSED = False
    try:
        gt, xt = _eikonal_step(m, x0)
        m64 = _net(dims, "relu", out, True, dev, seed=7).double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        g64, x64 = _eikonal_step(m64, x0.double(), torch.float64)
    finally:
        mlp_mod.USE_FUSED = True
    _check("x.grad", xf, x64.double(), xt)
    for i, (a, b, r) in enumerate(zip(gf, gt, g64)):
        _check(f"param {i}", a, r.double(), b)


def test_eikonal_step_through_the_half_block(dev):
    """the half block's second order is the fp32 network's (as its torch route): same step against MLP(dtype=float) on the fused
    and on the torch route"""
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    torch.manual_seed(11)
    m = MLP(35, 1, D=1, W=64, dtype=torch.half, device=dev)
    x0 = torch.randn(2000, 35, generator=torch.Generator(device="cpu").manual_seed(4)).to(dev)

    def step(fused):
        mlp_mod.FUSED_SECOND_ORDER = fused
        try:
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            y = m(x)
            nablas, = torch.autograd.grad(y[:, 0].float().sum(), x, create_graph=True)
            assert (type(nablas.grad_fn).__name__ == "FusedMLPBackwardFunctionBackward") == fused
            ((nablas.norm(dim=-1) - 1.0) ** 2).sum().backward()
            return [None if p.grad is None else p.grad.float().clone() for p in m.parameters()]
        finally:
            mlp_mod.FUSED_SECOND_ORDER = True
    gf, gt = step(True), step(False)
    # (the output bias has no path to the nablas: None on both routes)
    assert [a is None for a in gf] == [b is None for b in gt] == [False, False, False, True]
    for i, (a, b) in enumerate(zip(gf[:3], gt[:3])):
        assert torch.isfinite(a).all()
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5, msg=f"param {i}")


def test_fallbacks_stay_correct(dev):
    """a loss on the parameter gradients (gradients arrive on dW outputs), third order, and a network outside the fused range"""
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net([16, 32, 32, 4], "relu", None, True, dev, seed=5)
    x0 = torch.randn(513, 16, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)

    def grad_penalty():
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        gs = torch.autograd.grad(y.square().mean(), list(m.parameters()), create_graph=True)
        nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        (sum(g.square().sum() for g in gs) + nablas.square().mean()).backward()
        return [p.grad.clone() for p in m.parameters()] + [x.grad.clone()]

    def third_order():
        x = x0.clone().requires_grad_(True)
        y = m(x)
        nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        w = m.layers[0].weight
        gw, = torch.autograd.grad(nablas.square().sum(), w, create_graph=True)
        gww, = torch.autograd.grad(gw.square().sum(), w)
        return [gw.detach(), gww]

    fused = grad_penalty(), third_order()
    mlp_mod.USE_FUSED = False
    try:
        ref = grad_penalty(), third_order()
    finally:
        mlp_mod.USE_FUSED = True
    for a_list, b_list in zip(fused, ref):
        for a, b in zip(a_list, b_list):
            torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5)
    # outside the fused double backward's range (hidden width 128): the torch route, as before
    wide = _net([32, 128, 4], "relu", None, True, dev)
    assert not _desc(wide).second_order_fusable
    x = torch.randn(100, 32, device=dev, requires_grad=True)
    nablas, = torch.autograd.grad(wide(x)[:, 0].sum(), x, create_graph=True)
    nablas.square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in list(wide.parameters())[:-1])   # (the output bias: no path)


def test_sdf_chain_end_to_end(dev):
    """LoTDSDF.forward_sdf_nablas: fp32 LoTD forward_dydx -> MLP(32 + 3 -> 64 -> 1) -> create_graph grad -> backward_dydx ->
    eikonal + sdf loss; encoder and decoder gradients against the same chain with USE_FUSED = False"""
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    from nr3d_lib_amd.models.grid_encodings.lotd import LoTDEncoding, gen_ngp_cfg
    cfg = gen_ngp_cfg(log2_hashmap_size=14, min_res=8, num_levels=16)
    torch.manual_seed(2)
    enc = LoTDEncoding(3, lotd_cfg=dict(lod_res=cfg["lod_res"], lod_n_feats=cfg["lod_n_feats"], lod_types=cfg["lod_types"],
                                        hashmap_size=cfg["hashmap_size"]),
                       dtype=torch.float, device=dev, param_init_cfg={"type": "uniform", "bound": 0.5})
    assert enc.out_features == 32
    dec = MLP(35, 1, D=1, W=64, dtype=torch.float, device=dev)
    x0 = torch.rand(4000, 3, generator=torch.Generator(device="cpu").manual_seed(6)).to(dev) * 1.8 - 0.9

    def step():
        enc.zero_grad(set_to_none=True); dec.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        h, dy_dx = enc.forward_dydx(x)
        h_in = torch.cat([h, x], dim=-1)
        sdf = dec(h_in)[..., 0]
        dL_dh, = torch.autograd.grad(sdf, h_in, torch.ones_like(sdf), create_graph=True)
        nablas = enc.backward_dydx(dL_dh[..., :32].contiguous(), dy_dx, x) + dL_dh[..., 32:]
        loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + sdf.abs().mean()
        loss.backward()
        return [enc.flattened_params.grad.clone()] + [p.grad.clone() for p in dec.parameters()]
    gf = step()
    mlp_mod.USE_FUSED = False
    try:
        gt = step()
    finally:
        mlp_mod.USE_FUSED = True
    for i, (a, b) in enumerate(zip(gf, gt)):
        assert torch.isfinite(a).all()
        scale = float(b.abs().max()) or 1.0
        err = float((a - b).abs().max()) / scale
        assert err < 1e-4, f"gradient {i}: rel err {err:.2e}"


# (in, width, out) tiles and hidden layers of csrc/mlp.hip's BWD2_CASE table (NR3D_MLP_BWD_SHAPES, mlp_plan.h)
BWD_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (1, 2, 1, 1), (1, 2, 1, 2), (1, 2, 2, 1), (1, 2, 2, 2),
              (2, 2, 1, 1), (2, 2, 1, 2), (2, 2, 2, 1), (2, 2, 2, 2)]
_table_refs = {}


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_every_double_backward_table_entry(dev, hip_option, shape, x3):
    """k_mlp_bwd2<I, W, O, H, X3> for every shape of the table and both MFMA routes (shapes without a bf16 kernel run the f32 one
    under mlp_x3 = 1), launched once each: ragged widths (18 / 50 in, 3 / 33 out), x feature-major and ddL_dx row-major, n = 257
    (eight waves with a tile each + one partial tile + a second workgroup: the smallest size at which a wrong wave count, LDS size
    or grid of the launch plan shows) and n = 1"""
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    i, w, o, h = shape
    dims = [32 * i - 14] + [32 * w] * h + [32 * o - 29]
    m = _net(dims, "relu", None, True, dev, seed=21)
    d = _desc(m)
    assert d.second_order_fusable
    ws, bs = _params(m)
    packed = _mlp.pack(d, ws, bs, with_backward=True)
    for n in (257, 1):
        g = torch.Generator(device="cpu").manual_seed(100 + n)
        x = torch.randn(n, dims[0], generator=g).to(dev)
        gy = torch.randn(n, dims[-1], generator=g).to(dev)
        v = torch.randn(n, dims[0], generator=g).to(dev)
        if (shape, n) not in _table_refs:                  # computed once, shared by the two mlp_x3 cases
            _table_refs[(shape, n)] = (_double_reference(m, x, gy, v, torch.float64), _double_reference(m, x, gy, v, torch.float32))
        (ref64, ggy64), (ref32, ggy32) = _table_refs[(shape, n)]
        dgy, dWs, _ = _mlp.backward_backward(d, _layouts(x, "feature_major"), gy, v, packed, need_dgy=True)
        assert torch.isfinite(dgy).all()
        _check(f"n={n} dL/d(dL_dy)", dgy, ggy64, ggy32)
        for l, (a, r64, r32) in enumerate(zip(dWs, ref64, ref32)):
            _check(f"n={n} dW[{l}]", a, r64, r32)
