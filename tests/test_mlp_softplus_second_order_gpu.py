"""GPU: the fused double backward of softplus hidden layers (csrc/mlp_softplus2.hip k_mlp_bwd2_sp through bindings._mlp.backward_backward_softplus
and models.blocks.mlp.FusedMLPBackwardFunction under FUSED_SOFTPLUS_SECOND_ORDER) against torch's own double backward.

Yardstick, in the form of tests/test_mlp_second_order_gpu.py: the error against a float64 evaluation, relative to the tensor's maximum,
stays within max(1e-5, 8 x the error of torch's own fp32 evaluation of the same inputs).  The factor is 8 where the first-order tests
use 4: beta enters the second order twice, and an emulated independent fp32 evaluation of these formulas (z summed in another order,
exp / log at the hardware's accuracy) lands at up to 4.2 x torch's error; 8 is twice that.  Every check prints its ratio
("YARDSTICK ..."; profiles/mlp_softplus_second_order.json keeps one run of them: 584 checks, the largest ratio 4.5, the median 0.8).

All softplus networks use beta = 100 (one case: 5) and the 0.4 / 0.2 randn parameters of the other fused MLP tests.  The tests set
FUSED_SOFTPLUS_SECOND_ORDER themselves, so they cover the fused route whatever its default is."""
import contextlib

import pytest
import torch

from mlp_half_ref import check_rows_against_twin, double_twin
from mlp_softplus2_ref import torch_double_backward

pytestmark = pytest.mark.gpu

BETA = 100.0


@contextlib.contextmanager
def _switch(on=True, **others):
    """FUSED_SOFTPLUS_SECOND_ORDER = on (and any other module switch) for the block, restored afterwards"""
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    names = dict(FUSED_SOFTPLUS_SECOND_ORDER=on, **others)
    saved = {k: getattr(mlp_mod, k) for k in names}
    try:
        for k, val in names.items():
            setattr(mlp_mod, k, val)
        yield mlp_mod
    finally:
        for k, val in saved.items():
            setattr(mlp_mod, k, val)


def _net(dims, bias, dev, seed=0, beta=BETA, dtype=torch.float, out=None):
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(seed)
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=dict(type="softplus", beta=beta), output_activation=out, bias=bias,
            dtype=dtype, device=dev)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.4 if p.dim() > 1 else 0.2))
    return m


def _params(m):
    return [l.weight for l in m.layers], [l.bias for l in m.layers]


def _packed(m):
    from nr3d_lib_amd.bindings import _mlp
    d = m.fused_desc()
    assert d is not None and d.hidden_activation == _mlp.ACT_SOFTPLUS and d.softplus_second_order_fusable and not d.second_order_fusable
    return d, _mlp.pack(d, *_params(m), with_backward=True)


def _inputs(dims, n, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(n, dims[0], generator=g) * scale).to(dev)
    gy = torch.randn(n, dims[-1], generator=g).to(dev)
    v = torch.randn(n, dims[0], generator=g).to(dev)
    return x, gy, v


def _refs(m, x, gy, v):
    """torch's double backward in float64 and in fp32: ((dgy, dx, [dW], [db | None]), the same)"""
    ws, bs = _params(m)
    beta = float(m.layers[0].activation.beta)
    out_relu = m.layers[-1].activation is not None
    return (torch_double_backward(ws, bs, x, gy, v, beta, out_relu, torch.float64),
            torch_double_backward(ws, bs, x, gy, v, beta, out_relu, torch.float32))


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64.double()).abs().max()) / scale
    err32 = float((ref32.double() - ref64.double()).abs().max()) / scale
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(1e-5, 8 * err32), f"{name}: rel err {err:.2e} (torch fp32 path: {err32:.2e})"


def _check_all(tag, got, r64, r32, dgy=True, dx=True, bias=None):
    """got = backward_backward_softplus's (dgy, dx, [dW], [db]); bias[l] False: db[l] was not asked for"""
    if dgy:
        _check(f"{tag} dL/d(dL_dy)", got[0], r64[0], r32[0])
    if dx:
        _check(f"{tag} dL/dx", got[1], r64[1], r32[1])
    n_l = len(r64[2])
    for l in range(n_l):
        _check(f"{tag} dW[{l}]", got[2][l], r64[2][l], r32[2][l])
        if r64[3][l] is not None and (bias is None or bias[l]):
            _check(f"{tag} db[{l}]", got[3][l], r64[3][l], r32[3][l])
    if got[3][n_l - 1] is not None:
        assert not got[3][n_l - 1].any(), f"{tag}: the output bias gets nothing"


def _layouts(t, layout):
    """[n, w] -> the same values row-major, feature-major ([w, n] storage) or as rows with a padded stride (NaN in the padding)"""
    if layout == "feature_major":
        return t.t().contiguous().t()
    if layout == "strided":
        n, w = t.shape
        buf = torch.full((n, w + 5), float("nan"), device=t.device)
        buf[:, :w] = t
        return buf[:, :w]
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# every entry of the kernel table
# ------------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (1, 2, 1, 1), (1, 2, 1, 2), (1, 2, 2, 1), (1, 2, 2, 2),
              (2, 2, 1, 1), (2, 2, 1, 2), (2, 2, 2, 1), (2, 2, 2, 2)]             # (in, width, out) tiles, hidden layers
_table_refs = {}


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_every_softplus_double_backward_table_entry(dev, hip_option, shape, x3):
    """k_mlp_bwd2_sp<I, W, O, H, X3> for every shape of NR3D_MLP_BWD_SHAPES and both MFMA routes (shapes without a bf16 kernel run the
    f32 one under mlp_x3 = 1): ragged widths (18 / 50 in, 3 / 33 out), x feature-major and ddL_dx row-major, n = 257 (eight full tiles
    and a partial one: several workgroups at every wave count of the launch plan, the smallest size at which a wrong wave count, LDS
    size or grid shows) and n = 1; all four kinds of output, dL/dx feature-major"""
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    i, w, o, h = shape
    dims = [32 * i - 14] + [32 * w] * h + [32 * o - 29]
    m = _net(dims, True, dev, seed=21)
    d, packed = _packed(m)
    for n in (257, 1):
        x, gy, v = _inputs(dims, n, 100 + n, dev)
        if (shape, n) not in _table_refs:                  # computed once, shared by the two mlp_x3 cases
            _table_refs[(shape, n)] = _refs(m, x, gy, v)
        r64, r32 = _table_refs[(shape, n)]
        got = _mlp.backward_backward_softplus(d, _layouts(x, "feature_major"), gy, v, packed)
        assert n == 1 or got[1].stride() == (1, n)
        assert tuple(got[0].shape) == (n, dims[-1]) and tuple(got[1].shape) == (n, dims[0])
        _check_all(f"{shape} x3={x3} n={n}", got, r64, r32)


# ------------------------------------------------------------------------------------------------------------------------
# the binding
# ------------------------------------------------------------------------------------------------------------------------
CASES = [
    # dims, n, bias, output activation, beta
    ([35, 64, 1], 4099, True, None, BETA),
    ([32, 64, 64, 16], 1031, True, None, BETA),
    ([3, 8, 1], 1, True, None, BETA),
    ([16, 32, 32, 32, 7], 513, False, None, BETA),
    ([35, 40, 1], 257, False, None, BETA),               # padded hidden lanes: s = e = 1/2 there, g = t = 0
    ([18, 64, 3], 777, True, "relu", BETA),
    ([32, 64, 16], 257, True, None, 5.0),
]


@pytest.mark.parametrize("dims,n,bias,out,beta", CASES)
def test_binding_matches_torch_double_backward(dev, dims, n, bias, out, beta):
    from nr3d_lib_amd.bindings import _mlp
    m = _net(dims, bias, dev, seed=3, beta=beta, out=out)
    d, packed = _packed(m)
    assert d.beta == beta
    x, gy, v = _inputs(dims, n, 1, dev)
    r64, r32 = _refs(m, x, gy, v)
    n_l = len(dims) - 1
    hb = [bias] * n_l
    for layout in ("row", "feature_major", "strided"):
        got = _mlp.backward_backward_softplus(d, _layouts(x, layout), gy, _layouts(v, layout), packed, has_bias=hb)
        assert got[0].shape == gy.shape and got[1].shape == x.shape
        assert all((b is not None) == bias for b in got[3])
        if layout == "feature_major" and n > 1:
            assert got[1].stride() == (1, n)
        _check_all(f"{dims} {layout}", got, r64, r32)
    # outputs that are not asked for are None, the others unchanged within the yardstick
    got = _mlp.backward_backward_softplus(d, x, gy, v, packed, need_dgy=False, has_bias=hb)
    assert got[0] is None and got[1] is not None
    _check_all(f"{dims} need_dgy=False", got, r64, r32, dgy=False)
    got = _mlp.backward_backward_softplus(d, x, gy, v, packed, need_dx=False, has_bias=hb)
    assert got[1] is None and got[0] is not None
    _check_all(f"{dims} need_dx=False", got, r64, r32, dx=False)
    part = [bias and l % 2 == 1 for l in range(n_l)]
    got = _mlp.backward_backward_softplus(d, x, gy, v, packed, need_dgy=False, need_dx=False, has_bias=part)
    assert got[0] is None and got[1] is None and [b is not None for b in got[3]] == part
    _check_all(f"{dims} has_bias={part}", got, r64, r32, dgy=False, dx=False, bias=part)


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("dims", [[35, 64, 1], [32, 64, 64, 16]])
def test_binding_stride0_dL_dy_and_odd_n(dev, hip_option, x3, dims):
    """dL_dy as an expanded ones (row stride 0, what autograd hands the sdf column) and n = 1, 33, 100"""
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    m = _net(dims, True, dev, seed=3)
    d, packed = _packed(m)
    for n in (1, 33, 100):
        x, _, v = _inputs(dims, n, 2 + n, dev)
        gy = torch.ones(1, 1, device=dev).expand(n, dims[-1])
        r64, r32 = _refs(m, x, gy, v)
        got = _mlp.backward_backward_softplus(d, x, gy, v, packed)
        assert tuple(got[0].shape) == (n, dims[-1])
        _check_all(f"{dims} x3={x3} ones n={n}", got, r64, r32)


@pytest.mark.parametrize("x3", [0, 1])
def test_saturated_units_stay_finite(dev, hip_option, x3):
    """x * 40: beta z reaches +-1e4 -- s = 1, e = 0 above the threshold, s = 0 far below, no inf * 0 anywhere"""
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    dims = [32, 64, 64, 16]
    m = _net(dims, True, dev, seed=31)
    d, packed = _packed(m)
    x, gy, v = _inputs(dims, 1031, 32, dev, scale=40.0)
    with torch.no_grad():
        z1 = torch.nn.functional.linear(x.double(), m.layers[0].weight.double(), m.layers[0].bias.double())
        assert float(z1.max()) > 100.0 and float(z1.min()) < -100.0
    r64, r32 = _refs(m, x, gy, v)
    _check_all(f"saturated x3={x3}", _mlp.backward_backward_softplus(d, x, gy, v, packed), r64, r32)


def test_each_binding_refuses_the_other_activation(dev):
    from nr3d_lib_amd.bindings import _mlp
    x, gy, v = _inputs([35, 64, 1], 33, 1, dev)
    sp = _net([35, 64, 1], True, dev)
    d, packed = _packed(sp)
    with pytest.raises(RuntimeError):
        _mlp.backward_backward(d, x, gy, v, packed)
    relu = _mlp.MLPDesc([35, 64, 1], _mlp.ACT_RELU, _mlp.ACT_NONE)
    assert relu.second_order_fusable and not relu.softplus_second_order_fusable
    packed_r = _mlp.pack(relu, *_params(sp), with_backward=True)
    with pytest.raises(RuntimeError):
        _mlp.backward_backward_softplus(relu, x, gy, v, packed_r)
    # ... and so does the C entry, with a message
    import ctypes as C
    from nr3d_lib_amd import _hip as H
    rc = H.lib().nr3d_mlp_softplus_backward_backward(C.byref(relu._c), 33, H.ptr(x), 35, 1, H.ptr(gy), 1, H.ptr(v), 35, 1, H.ptr(packed_r),
                                                     None, 1, None, 35, 1, None, None, None)
    assert rc != 0 and b"softplus" in H.lib().nr3d_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# autograd
# ------------------------------------------------------------------------------------------------------------------------
def test_create_graph_routes_through_the_fused_double_backward(dev):
    from nr3d_lib_amd.bindings import _mlp
    m = _net([35, 64, 1], True, dev, seed=1)
    x = torch.randn(1000, 35, device=dev, requires_grad=True)
    with _switch(True):
        nablas, = torch.autograd.grad(m(x)[:, 0].sum(), x, create_graph=True)
        assert type(nablas.grad_fn).__name__ == "FusedMLPBackwardFunctionBackward"
        d, packed = _packed(m)
        dx, _, _ = _mlp.backward(d, x.detach(), torch.ones(1000, 1, device=dev), packed)
        assert torch.equal(nablas, dx)
        # the eikonal term alone: x and the hidden biases get a non-zero gradient, the output bias None
        m.zero_grad(set_to_none=True)
        ((nablas.norm(dim=-1) - 1.0) ** 2).mean().backward()
        assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
        assert m.layers[0].bias.grad is not None and float(m.layers[0].bias.grad.abs().max()) > 0
        assert float(m.layers[0].weight.grad.abs().max()) > 0 and float(m.layers[1].weight.grad.abs().max()) > 0
        assert m.layers[1].bias.grad is None
    with _switch(False):
        nablas_t, = torch.autograd.grad(m(x)[:, 0].sum(), x, create_graph=True)
    assert type(nablas_t.grad_fn).__name__ != "FusedMLPBackwardFunctionBackward"
    torch.testing.assert_close(nablas_t, nablas, rtol=1e-4, atol=1e-5)
    with _switch(True, FUSED_SECOND_ORDER=False):
        nablas_t, = torch.autograd.grad(m(x)[:, 0].sum(), x, create_graph=True)
    assert type(nablas_t.grad_fn).__name__ != "FusedMLPBackwardFunctionBackward"
    # an output ReLU: its bias reaches the nablas through the mask only -- zeros, as on the torch route
    mr = _net([18, 64, 3], True, dev, seed=2, out="relu")
    xr = torch.randn(257, 18, device=dev, requires_grad=True)
    with _switch(True):
        nablas, = torch.autograd.grad(mr(xr)[:, 0].sum(), xr, create_graph=True)
        assert type(nablas.grad_fn).__name__ == "FusedMLPBackwardFunctionBackward"
        nablas.square().sum().backward()
    assert mr.layers[1].bias.grad is not None and not mr.layers[1].bias.grad.any()
    assert float(mr.layers[0].bias.grad.abs().max()) > 0


def _eikonal_step(m, x0, dt=torch.float32):
    m.zero_grad(set_to_none=True)
    x = x0.to(dt).clone().requires_grad_(True)
    y = m(x)
    nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
    loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + y.square().mean()
    loss.backward()
    return [p.grad.clone() for p in m.parameters()], x.grad.clone(), type(nablas.grad_fn).__name__


def _double_twin(m, dims, bias, dev, out=None):
    m64 = _net(dims, bias, dev, out=out).double()
    m64.load_state_dict({k: val.double() for k, val in m.state_dict().items()})
    return m64


@pytest.mark.parametrize("dims,out", [([35, 64, 1], None), ([32, 64, 64, 16], None), ([16, 32, 32, 4], None)])
def test_eikonal_step_matches_torch_and_float64(dev, dims, out):
    """eikonal + sdf loss: x.grad and every parameter of the fused route against the same module in float64, the USE_FUSED = False
    fp32 run as the yardstick's reference"""
    m = _net(dims, True, dev, seed=7, out=out)
    x0 = torch.randn(3000, dims[0], generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    with _switch(True):
        gf, xf, fn = _eikonal_step(m, x0)
    assert fn == "FusedMLPBackwardFunctionBackward"
    with _switch(True, USE_FUSED=False):
        gt, xt, fn = _eikonal_step(m, x0)
        assert fn != "FusedMLPBackwardFunctionBackward"
        g64, x64, _ = _eikonal_step(_double_twin(m, dims, True, dev, out), x0.double(), torch.float64)
    _check(f"{dims} x.grad", xf, x64, xt)
    for i, (a, b, r) in enumerate(zip(gf, gt, g64)):
        _check(f"{dims} param {i}", a, r, b)


def test_eikonal_step_through_the_half_block(dev):
    """the half block's second order is the fp32 network's: fused against USE_FUSED = False as in
    test_second_order_through_the_half_softplus_block (tests/test_mlp_softplus_gpu.py) -- softplus has no kink, so EVERY row of the
    nablas and of x.grad is held to max(2e-2, 4 x the USE_FUSED = False run's worst row) of the tensor's scale against an fp64 twin of
    the module (parameters and x rounded to half, everything else double); the earlier comparison with the USE_FUSED = False run
    itself stays beside it.  Measured on an MI355X, worst row as a fraction of scale, fused (USE_FUSED = False): nablas 1.3e-3 (3.7e-4),
    x.grad 9.6e-3 (7.1e-4) -- 2e-2 is the bound in force."""
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(11)
    m = MLP(35, 1, D=1, W=64, activation=dict(type="softplus", beta=BETA), dtype=torch.half, device=torch.device("cpu")).to(dev)
    twin = double_twin(m)
    x0 = torch.randn(2000, 35, generator=torch.Generator(device="cpu").manual_seed(4)).to(dev)

    def run():
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        nablas, = torch.autograd.grad(y[:, 0].float().sum(), x, create_graph=True)
        (((nablas.float().norm(dim=-1) - 1.0) ** 2).sum() + y.float().square().sum()).backward()
        return (nablas.detach().float(), [p.grad.float().clone() for p in m.parameters()], x.grad.float().clone(),
                type(nablas.grad_fn).__name__)
    with _switch(True):
        nh, gh, xh, fn = run()
    assert fn == "FusedMLPBackwardFunctionBackward"
    with _switch(True, USE_FUSED=False):
        nr, gr, xr, fn = run()
    assert fn != "FusedMLPBackwardFunctionBackward"

    twin.zero_grad(set_to_none=True)
    x = x0.half().double().requires_grad_(True)
    y = twin(x)
    n64, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
    (((n64.norm(dim=-1) - 1.0) ** 2).sum() + y.square().sum()).backward()

    def rows_off(a, b, tol=2e-2):
        return float(((a - b).abs().amax(1) > tol * float(b.abs().max())).float().mean())
    assert torch.isfinite(nh).all() and torch.isfinite(xh).all()
    check_rows_against_twin("nablas", nh, nr, n64.detach())
    check_rows_against_twin("x.grad", xh, xr, x.grad)
    assert rows_off(nh, nr) < 0.05, f"nablas: {rows_off(nh, nr):.3f} of the rows differ"
    assert rows_off(xh, xr) < 0.05, f"x.grad: {rows_off(xh, xr):.3f} of the rows differ"
    for i, (a, b) in enumerate(zip(gh, gr)):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, f"param {i}"
        err = float((a - b).norm() / b.norm())
        print(f"half block param {i}: relative difference {err:.3e}")
        assert err < 5e-2, f"param {i}: relative difference of the gradient {err:.3e}"


def test_fallbacks_stay_correct(dev):
    """gradients arriving on dW outputs (a penalty on the parameter gradients) and third order still differentiate the torch
    evaluation: fused block against the same module in float64, the USE_FUSED = False fp32 run as the yardstick's reference"""
    dims = [16, 32, 32, 4]
    m = _net(dims, True, dev, seed=5)
    x0 = torch.randn(513, 16, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)

    def grad_penalty(net, dt):
        net.zero_grad(set_to_none=True)
        x = x0.to(dt).clone().requires_grad_(True)
        y = net(x)
        gs = torch.autograd.grad(y.square().mean(), list(net.parameters()), create_graph=True)
        nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        (sum(g.square().sum() for g in gs) + nablas.square().mean()).backward()
        return [p.grad.clone() for p in net.parameters()] + [x.grad.clone()]

    def third_order(net, dt):
        x = x0.to(dt).clone().requires_grad_(True)
        y = net(x)
        nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        w = net.layers[0].weight
        gw, = torch.autograd.grad(nablas.square().sum(), w, create_graph=True)
        gww, = torch.autograd.grad(gw.square().sum(), w)
        return [gw.detach(), gww]

    with _switch(True):
        fused = grad_penalty(m, torch.float32) + third_order(m, torch.float32)
    with _switch(True, USE_FUSED=False):
        ref32 = grad_penalty(m, torch.float32) + third_order(m, torch.float32)
        m64 = _double_twin(m, dims, True, dev)
        ref64 = grad_penalty(m64, torch.float64) + third_order(m64, torch.float64)
    for i, (a, b, r) in enumerate(zip(fused, ref32, ref64)):
        _check(f"fallback {i}", a, r, b)


def test_sdf_chain_end_to_end(dev):
    """LoTDSDF.forward_sdf_nablas with a softplus decoder: fp32 LoTD forward_dydx -> MLP(32 + 3 -> 64 -> 1, softplus) -> create_graph
    grad -> backward_dydx -> eikonal + sdf loss.  Encoder and decoder gradients of the fused route against the chain whose decoder runs
    in float64 (the encoder kernels are fp32 in all three), the USE_FUSED = False fp32 chain as the yardstick's reference"""
    from nr3d_lib_amd.models.grid_encodings.lotd import LoTDEncoding, gen_ngp_cfg
    cfg = gen_ngp_cfg(log2_hashmap_size=14, min_res=8, num_levels=16)
    torch.manual_seed(2)
    enc = LoTDEncoding(3, lotd_cfg=dict(lod_res=cfg["lod_res"], lod_n_feats=cfg["lod_n_feats"], lod_types=cfg["lod_types"],
                                        hashmap_size=cfg["hashmap_size"]),
                       dtype=torch.float, device=dev, param_init_cfg={"type": "uniform", "bound": 0.5})
    assert enc.out_features == 32
    dec = _net([35, 64, 1], True, dev, seed=9)
    x0 = torch.rand(4000, 3, generator=torch.Generator(device="cpu").manual_seed(6)).to(dev) * 1.8 - 0.9

    def step(net, dt=torch.float32):
        enc.zero_grad(set_to_none=True); net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        h, dy_dx = enc.forward_dydx(x)
        h_in = torch.cat([h, x], dim=-1).to(dt)
        sdf = net(h_in)[..., 0]
        dL_dh, = torch.autograd.grad(sdf, h_in, torch.ones_like(sdf), create_graph=True)
        fn = type(dL_dh.grad_fn).__name__
        dL_dh = dL_dh.float()
        nablas = enc.backward_dydx(dL_dh[..., :32].contiguous(), dy_dx, x) + dL_dh[..., 32:]
        loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + sdf.float().abs().mean()
        loss.backward()
        return [enc.flattened_params.grad.clone()] + [p.grad.clone() for p in net.parameters()], fn
    with _switch(True):
        gf, fn = step(dec)
    assert fn == "FusedMLPBackwardFunctionBackward"
    with _switch(True, USE_FUSED=False):
        gt, fn = step(dec)
        assert fn != "FusedMLPBackwardFunctionBackward"
        g64, _ = step(_double_twin(dec, [35, 64, 1], True, dev), torch.float64)
    for i, (a, b, r) in enumerate(zip(gf, gt, g64)):
        _check(f"sdf chain gradient {i}", a, r, b)
