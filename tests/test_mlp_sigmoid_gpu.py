"""GPU: the sigmoid output activation on the fused MLP kernels (csrc/mlp.hip, csrc/mlp_half.hip, csrc/mlp_act.h through bindings._mlp /
models.blocks.MLP) against torch evaluations in float64 on the tests' own tensors -- the radiance decoders of the reference:
MLP(32, 3, D=2, W=64, activation='relu', output_activation='sigmoid').

fp32: the yardstick of tests/test_mlp_softplus_gpu.py -- the error against fp64 stays within max(1e-5 of the output scale, 4 x the
error of torch's own fp32 evaluation), for y, dL/dx and every dW / db.  Half: the rounded-contract fp64 reference (sigmoid on the
unrounded output accumulator, then one rounding; tests/mlp_half_ref.py) at 2^-9 of scale for y, 2^-7 for gradients (4 x that for dW /
db when n < 100); dL/dx row by row: every row within 2^-7, or proven to sit on a kink of a ReLU hidden layer (assert_rows there; at
most max(2, n // 2000) rows).  tests/test_mlp_sigmoid_cpu.py: no row depends on the order of rounding and sigmoid at the output.

The last layer's weights have scale 0.1, not the 0.4 of the other test files: most outputs then sit in the sigmoid's active range and
sigma' matters (at 0.4 about half of them saturate).  Nearly every case has padded output columns (out_dim = 3, 1, 33: sigmoid(0) =
0.5 with derivative 0.25 in them, where a ReLU / linear output has 0) and the FAST table entries have rows past n."""
import ctypes as C

import pytest
import torch

from mlp_half_ref import assert_rows, fill_parameters, half_contract, max_excused

pytestmark = pytest.mark.gpu

BETA = 100.0
SOFTPLUS = dict(type="softplus", beta=BETA)


def _net(dims, bias, dev, hidden="relu", seed=0, dtype=torch.float, last_scale=0.1):
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(seed)
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=hidden or "none", output_activation="sigmoid", bias=bias,
            dtype=dtype, device=dev)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.4 if p.dim() > 1 else 0.2))
        m.layers[-1].weight.mul_(last_scale / 0.4)
    return m


def _activate(layer, h):
    a = layer.activation
    if a is None:
        return h
    if isinstance(a, torch.nn.Sigmoid):
        return torch.sigmoid(h)
    if isinstance(a, torch.nn.Softplus):
        return torch.nn.functional.softplus(h, a.beta, a.threshold)
    assert isinstance(a, torch.nn.ReLU), a
    return torch.relu(h)


def _reference(m, x, gy, dtype):
    """layer-by-layer torch evaluation in `dtype` -> (y, dx, [dW], [db])"""
    h = x.detach().to(dtype).requires_grad_(True)
    h0 = h
    ws = [l.weight.detach().to(dtype).requires_grad_(True) for l in m.layers]
    bs = [None if l.bias is None else l.bias.detach().to(dtype).requires_grad_(True) for l in m.layers]
    for l, W, b in zip(m.layers, ws, bs):
        h = _activate(l, torch.nn.functional.linear(h, W, b))
    h.backward(gy.to(dtype))
    return h.detach(), h0.grad, [w.grad for w in ws], [None if b is None else b.grad for b in bs]


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64).abs().max()) / scale
    err32 = float((ref32.double() - ref64).abs().max()) / scale
    print(f"{name}: rel err {err:.2e} (torch fp32 path: {err32:.2e})")
    assert torch.isfinite(got).all() and err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 path: {err32:.2e})"


def _check_all(tag, m, y, dx, dWs, dbs, r64, r32):
    _check(f"{tag} y", y, r64[0], r32[0])
    _check(f"{tag} dL_dx", dx, r64[1], r32[1])
    for l in range(len(m.layers)):
        _check(f"{tag} dL_dW{l}", dWs[l], r64[2][l], r32[2][l])
        if r64[3][l] is not None:
            _check(f"{tag} dL_db{l}", dbs[l], r64[3][l], r32[3][l])


# ------------------------------------------------------------------------------------------------------------------------
# fp32, module level
# ------------------------------------------------------------------------------------------------------------------------
CASES = [
    # dims, n, bias, hidden
    ([32, 64, 64, 3], 4099, True, "relu"),          # the LoTD NeRF radiance decoder of the reference
    ([31, 64, 3], 257, True, "relu"),
    ([3, 8, 1], 1, True, "relu"),
    ([16, 32, 32, 32, 3], 513, False, "relu"),
    ([35, 40, 33], 257, False, None),               # two output tiles, 31 padded columns at 0.5; padded hidden columns
    ([35, 64, 3], 1031, True, SOFTPLUS),
]


@pytest.mark.parametrize("dims,n,bias,hidden", CASES)
def test_sigmoid_block_matches_torch(dev, dims, n, bias, hidden):
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net(dims, bias, dev, hidden)
    desc = m.fused_desc()
    assert desc is not None and desc.output_activation == _mlp.ACT_SIGMOID and desc.backward_fusable
    assert desc.hidden_activation == (_mlp.ACT_SOFTPLUS if hidden is SOFTPLUS else _mlp.ACT_RELU if hidden else _mlp.ACT_NONE)
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(n, dims[0], generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(n, dims[-1], generator=g).to(dev)
    r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
    y = m(x)
    assert y.grad_fn is not None and "FusedMLPFunction" in type(y.grad_fn).__name__
    y.backward(gy)
    _check_all("fused", m, y.detach(), x.grad, [l.weight.grad for l in m.layers], [l.bias.grad if bias else None for l in m.layers], r64, r32)
    with torch.no_grad():
        _check("y (no_grad)", m(x), r64[0], r32[0])
    mlp_mod.USE_FUSED = False
    try:
        yu = m(x)
        assert "FusedMLP" not in type(yu.grad_fn).__name__
        _check("unfused y", yu.detach(), r64[0], r32[0])
    finally:
        mlp_mod.USE_FUSED = True


# ------------------------------------------------------------------------------------------------------------------------
# fp32, every entry of the backward table (csrc/mlp.hip BWD_CASE over NR3D_MLP_BWD_SHAPES x FAST x the bf16 route) with a sigmoid
# output, and the forward's XF / X3 selection with the same inputs.  fast 0: ragged widths; 1: whole tiles, prefetched rows (rows past
# n are clamped rows whose dL/dy is zeroed before it meets sigma'); 2: the same with a feature-major x
# ------------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (1, 2, 1, 1), (1, 2, 1, 2), (1, 2, 2, 1), (1, 2, 2, 2),
              (2, 2, 1, 1), (2, 2, 1, 2), (2, 2, 2, 1), (2, 2, 2, 2)]             # (in, width, out) tiles, hidden layers
TABLE_NS = (257, 33, 1)


def _table_dims(shape, fast):
    """fast 0: ragged widths (dL/dy rows of 3 / 35 elements have no aligned pieces); 1, 2: whole tiles"""
    i, w, o, h = shape
    return [32 * i - 14 if fast == 0 else 32 * i] + [32 * w] * h + [32 * o - 29 if fast == 0 else 32 * o]


def _table_inputs(dims, n, fast, dev):
    g = torch.Generator(device="cpu").manual_seed(100 + n)
    x = torch.randn(n, dims[0], generator=g).to(dev)
    gy = torch.randn(n, dims[-1], generator=g).to(dev)
    return (x.t().contiguous().t() if fast == 2 else x), gy


_table_refs = {}


def _table_reference(key, m, x, gy):
    """fp64 and fp32 torch evaluations of one (shape, fast, n): computed once, shared by the two mlp_x3 cases"""
    if key not in _table_refs:
        _table_refs[key] = (_reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32))
    return _table_refs[key]


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("fast", [0, 1, 2])
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_every_fp32_backward_table_entry_with_a_sigmoid_output(dev, hip_option, shape, fast, x3):
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    dims = _table_dims(shape, fast)
    m = _net(dims, True, dev, seed=21)
    desc = m.fused_desc()
    assert desc is not None and desc.output_activation == _mlp.ACT_SIGMOID and desc.backward_fusable
    packed = _mlp.pack(desc, [l.weight for l in m.layers], [l.bias for l in m.layers], with_backward=True)
    for n in TABLE_NS:
        x, gy = _table_inputs(dims, n, fast, dev)
        r64, r32 = _table_reference((shape, fast, n), m, x, gy)
        y = _mlp.forward(desc, x, packed)
        dx, dWs, dbs = _mlp.backward(desc, x, gy, packed, need_dx=True)
        assert n == 1 or fast != 2 or dx.stride() == (1, n)
        _check_all(f"n={n}", m, y, dx, dWs, dbs, r64, r32)


# ------------------------------------------------------------------------------------------------------------------------
# half precision on the f16 MFMA (csrc/mlp_half.hip): MLP(dtype=torch.half) with a sigmoid output
# ------------------------------------------------------------------------------------------------------------------------
# 64-wide hidden layers run k_mlph_bwd_split (one and two of them, one and two input / output tiles), 32-wide ones k_mlph_bwd -- by the
# launch plan of csrc/mlp_half.hip (bwd_plan_of: w_t == 2 -> the split kernel); the binding does not report which kernel ran
HALF_CASES = [([32, 64, 64, 3], 4099), ([31, 64, 3], 257), ([16, 32, 32, 32, 3], 513), ([64, 64, 64, 64], 1031), ([3, 8, 1], 1)]


def half_net(dims, dev, last_scale=0.1):
    """weights from a CPU generator: the same net on the CPU (tests/test_mlp_sigmoid_cpu.py) and on the device"""
    m = fill_parameters(_net(dims, True, dev, "relu", seed=0, dtype=torch.half), 0)
    with torch.no_grad():
        m.layers[-1].weight.mul_(last_scale / 0.4)
    return m


def half_inputs(dims, n, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    return torch.randn(n, dims[0], generator=g).to(dev), torch.randn(n, dims[-1], generator=g).to(dev)


def _check_half(name, got, ref64, tol):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64).abs().max()) / scale
    print(f"{name}: rel err {err:.2e} (tol {tol:.2e})")
    assert torch.isfinite(got).all() and err <= tol, f"{name}: rel err {err:.2e} > {tol:.2e}"


def _half_run_and_check(m, dims, n, xs, gy, layout):
    if layout == "feature_major":
        xt = xs.t().contiguous().requires_grad_(True)
        x = xt.t()
    else:
        xt = x = xs.clone().requires_grad_(True)
    contract = half_contract(m, x, gy)
    y64, dx64, dW64, db64, _ = contract
    y = m(x)
    assert y.dtype == torch.float16 and "FusedMLPHalfFunction" in type(y.grad_fn).__name__
    y.backward(gy.half())
    _check_half("y", y.detach(), y64, 2.0 ** -9)
    with torch.no_grad():
        _check_half("y (no_grad)", m(x), y64, 2.0 ** -9)
    tol = 2.0 ** -7
    gx = (xt.grad.t() if layout == "feature_major" else xt.grad)
    assert gx.dtype == torch.float32 and gx.shape == dx64.shape and torch.isfinite(gx).all()
    assert_rows("dL_dx", gx, m, x, gy, tol, max_excused=max_excused(n), contract=contract)
    for l, layer in enumerate(m.layers):
        assert layer.weight.grad.dtype == torch.float32
        _check_half(f"dL_dW{l}", layer.weight.grad, dW64[l], 4 * tol if n < 100 else tol)
        _check_half(f"dL_db{l}", layer.bias.grad, db64[l], 4 * tol if n < 100 else tol)
    return y.detach(), gx, y64, dx64, dW64, db64


@pytest.mark.parametrize("layout", ["row_major", "feature_major"])
@pytest.mark.parametrize("dims,n", HALF_CASES)
def test_half_sigmoid_forward_backward(dev, dims, n, layout):
    """a pre-activation within rounding of a ReLU kink flips a unit between the kernel (fp32 accumulation) and the fp64 reference: as in
    test_half_fused_forward_backward, every row of dL/dx is within 2^-7 of scale or its kink is proven (assert_rows), for at most
    max(2, n // 2000) rows; dW / db are sums over rows"""
    from nr3d_lib_amd.bindings import _mlp
    m = half_net(dims, dev)
    desc = m.fused_desc()
    assert desc is not None and desc.output_activation == _mlp.ACT_SIGMOID and desc.half_fusable and desc.half_backward_fusable
    xs, gy = half_inputs(dims, n, dev)
    _half_run_and_check(m, dims, n, xs, gy, layout)


def test_half_sigmoid_agrees_with_the_autocast_layers(dev):
    """test_half_fused_agrees_with_the_autocast_layers on the radiance decoder: the same module with USE_FUSED off runs DenseLayer under
    autocast (half GEMMs, torch.sigmoid on the half output); the fused half kernels agree with it to half precision"""
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    torch.manual_seed(3)
    m = MLP(32, 3, D=2, W=64, activation="relu", output_activation="sigmoid", dtype=torch.half, device=dev)
    assert m.fused_desc() is not None
    x = torch.randn(20000, 32, device=dev)
    gy = torch.randn(20000, 3, device=dev).half()
    outs = {}
    for fused in (True, False):
        mlp_mod.USE_FUSED = fused
        try:
            m.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            y = m(xr)
            assert ("FusedMLPHalfFunction" in type(y.grad_fn).__name__) == fused
            y.backward(gy)
            outs[fused] = (y.detach().float(), xr.grad.float(), [l.weight.grad.clone() for l in m.layers])
        finally:
            mlp_mod.USE_FUSED = True
    scale = float(outs[False][0].abs().max())
    assert float((outs[True][0] - outs[False][0]).abs().max()) <= 2.0 ** -8 * scale
    for a, b in zip(outs[True][2], outs[False][2]):
        assert float((a - b).abs().max()) <= 2.0 ** -6 * float(b.abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# saturation: |z| of the output layer up to 1e3 .. 1e4
# ------------------------------------------------------------------------------------------------------------------------
SAT_DIMS, SAT_N = [32, 64, 3], 257
SAT_SCALE, SAT_BIAS = 15.0, (3000.0, -3000.0, 0.0)
# fp64's own sigmoid' = y (1 - y) is 0 by CANCELLATION from z = 36.7 on (y rounds to 1) although the true value, E / (1 + E)^2 = 1e-16 ..
# 1e-45, is a normal or denormal fp32 number, which the fp32 kernels keep as far as the hardware exp does.  "0 where float64 has 0" is
# therefore asked of the rows of dL/dx in which fp64's zeros are true ones: no output pre-activation inside this band.  (The half
# kernels round sigma' dL/dy to half, which is 0 from z = 17 on: every row is asked there.)
SAT_BAND = (36.0, 105.0)


def sat_net(dev, dtype):
    """weights from a CPU generator (the same on every machine): hidden layer at the usual 0.4 / 0.2, the output layer's weights at
    SAT_SCALE, 150 x the scale of the other tests -- W h has a standard deviation of about 200 -- and its bias at +3e3, -3e3 and 0:
    |z| is 2.4e3 .. 3.6e3 in the first two columns of every row, with either sign, and the third column runs through the sigmoid's
    whole range, with about two dozen of its 257 elements inside |z| < 15.  Those carry the whole gradient; many more of them would
    need a smaller spread, and fewer (a larger spread) leave a yardstick that compares two maxima over a handful of elements"""
    from nr3d_lib_amd.models.blocks import MLP
    m = MLP(SAT_DIMS[0], SAT_DIMS[-1], D=1, W=SAT_DIMS[1], activation="relu", output_activation="sigmoid", dtype=dtype, device=dev)
    g = torch.Generator(device="cpu").manual_seed(41)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.4 if p.dim() > 1 else 0.2))
        m.layers[-1].weight.mul_(SAT_SCALE / 0.4)
        m.layers[-1].bias.copy_(torch.tensor(SAT_BIAS))
    return m


def sat_inputs(dev):
    g = torch.Generator(device="cpu").manual_seed(42)
    return torch.randn(SAT_N, SAT_DIMS[0], generator=g).to(dev), torch.randn(SAT_N, SAT_DIMS[-1], generator=g).to(dev)


def sat_z(m, x, half):
    """the output layer's pre-activations in fp64 (half: of the rounded contract)"""
    rnd = (lambda t: t.half().double()) if half else (lambda t: t.double())
    with torch.no_grad():
        h = rnd(x)
        for l in m.layers[:-1]:
            h = rnd(torch.relu(torch.nn.functional.linear(h, rnd(l.weight), rnd(l.bias))))
        return torch.nn.functional.linear(h, rnd(m.layers[-1].weight), rnd(m.layers[-1].bias))


def _zero_where_fp64_is_zero(name, got, ref64):
    z = ref64 == 0
    assert bool((got[z] == 0).all()), f"{name}: {int((got[z] != 0).sum())} of {int(z.sum())} elements are not 0 where float64 has 0"
    return int(z.sum())


@pytest.mark.parametrize("x3", [0, 1])
def test_saturated_sigmoid_fp32(dev, hip_option, x3):
    """E = exp(-|z|) is 0 at |z| = 1e3 .. 1e4: y exactly 1 / 0, sigma' exactly 0, no inf * 0, nothing non-finite; the unsaturated
    elements of the third column carry the whole gradient and stay within the yardstick"""
    hip_option("mlp_x3", x3)
    m = sat_net(dev, torch.float)
    assert m.fused_desc() is not None
    xs, gy = sat_inputs(dev)
    z = sat_z(m, xs, False)
    assert float((z.abs().amax(1) > 1e3).float().mean()) > 0.5 and float(z.abs().max()) < 1e4 and float(z.max()) > 1e3 and float(z.min()) < -1e3
    x = xs.clone().requires_grad_(True)
    r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
    y = m(x)
    assert "FusedMLPFunction" in type(y.grad_fn).__name__
    y.backward(gy)
    _check_all(f"x3={x3}", m, y.detach(), x.grad, [l.weight.grad for l in m.layers], [l.bias.grad for l in m.layers], r64, r32)
    ones, zeros = r64[0] == 1, r64[0] == 0
    assert int(ones.sum()) > 200 and int(zeros.sum()) > 200
    assert bool((y.detach()[ones] == 1).all()) and bool((y.detach()[zeros] == 0).all())
    true_zero = (r64[1] == 0).all(1) & ~((z > SAT_BAND[0]) & (z < SAT_BAND[1])).any(1)
    print(f"rows of dL/dx that are 0 in float64: {int((r64[1] == 0).all(1).sum())}, with no z in the band: {int(true_zero.sum())}")
    assert int(true_zero.sum()) > 20
    assert bool((x.grad[true_zero] == 0).all()), f"{int((x.grad[true_zero] != 0).any(1).sum())} rows of dL/dx are not 0 where float64 has 0"
    # the saturated columns' rows of the output layer's dW / db are sums of exact zeros (|z| > 2e3: far outside the band)
    n_zero = 0
    for l, layer in enumerate(m.layers):
        n_zero += _zero_where_fp64_is_zero(f"dL_dW{l}", layer.weight.grad, r64[2][l]) + _zero_where_fp64_is_zero(f"dL_db{l}", layer.bias.grad, r64[3][l])
    assert n_zero >= 2 * (SAT_DIMS[1] + 1)


@pytest.mark.parametrize("layout", ["row_major", "feature_major"])
def test_saturated_sigmoid_half(dev, layout):
    m = sat_net(dev, torch.half)
    assert m.fused_desc() is not None and m.fused_desc().half_backward_fusable
    xs, gy = sat_inputs(dev)
    z = sat_z(m, xs, True)
    assert float((z.abs().amax(1) > 1e3).float().mean()) > 0.5 and float(z.abs().max()) < 1e4
    y, gx, y64, dx64, dW64, db64 = _half_run_and_check(m, SAT_DIMS, SAT_N, xs, gy, layout)
    ones, zeros = y64 == 1, y64 == 0
    assert int(ones.sum()) > 200 and int(zeros.sum()) > 200
    assert bool((y[ones] == 1).all()) and bool((y[zeros] == 0).all())
    _zero_where_fp64_is_zero("dL_dx", gx, dx64)
    for l, layer in enumerate(m.layers):
        _zero_where_fp64_is_zero(f"dL_dW{l}", layer.weight.grad, dW64[l])
        _zero_where_fp64_is_zero(f"dL_db{l}", layer.bias.grad, db64[l])


# ------------------------------------------------------------------------------------------------------------------------
# forward_columns: the sub-descriptor carries the sigmoid
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float, torch.half])
def test_forward_columns_carries_the_sigmoid(dev, hip_option, dtype):
    """fp32: the first column of the sigmoid output, bit for bit the full call's; half: the same through the 4-column rule of
    MLP.forward_columns (here min(3, 4) = all three columns are computed and the view drops two)"""
    m = _net([32, 64, 64, 3], True, dev, seed=5, dtype=dtype)
    assert m.fused_desc() is not None
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(1031, 32, generator=g).to(dev).to(dtype)
    for x3 in ((1, 0) if dtype == torch.float else (1,)):
        hip_option("mlp_x3", x3)
        with torch.no_grad():
            full = m(x)
            part = m.forward_columns(x, 1)
        assert tuple(part.shape) == (1031, 1) and part.dtype == full.dtype and torch.isfinite(full).all()
        assert float(full.min()) >= 0 and float(full.max()) <= 1 and float(full.max()) - float(full.min()) > 0.5
        assert torch.equal(part, full[:, :1]), f"x3={x3}"


# ------------------------------------------------------------------------------------------------------------------------
# second order: no fused double backward through a sigmoid output -- the create_graph backward differentiates the torch evaluation
# ------------------------------------------------------------------------------------------------------------------------
def _clone(g):
    return None if g is None else g.float().clone()


@pytest.mark.parametrize("hidden", ["relu", "softplus"])
def test_second_order_through_the_sigmoid_block(dev, hidden):
    """the eikonal pattern of test_second_order_through_the_softplus_block: fused block against USE_FUSED = False at that test's
    tolerances.  The first-order nablas (no create_graph) are the fused backward kernel's dL/dx bit for bit; with create_graph they come
    from the torch evaluation of the same network, since neither double backward kernel takes a sigmoid output"""
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net([16, 32, 32, 3], True, dev, SOFTPLUS if hidden == "softplus" else "relu", seed=5)
    desc = m.fused_desc()
    assert desc is not None and desc.backward_fusable and not desc.second_order_fusable and not desc.softplus_second_order_fusable
    assert not mlp_mod._fused_second_order(desc)
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(513, 16, generator=g).to(dev)

    def run():
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
        assert nablas.requires_grad
        eik = ((nablas.norm(dim=-1) - 1.0) ** 2).mean()
        (eik + y.square().mean()).backward()
        return y.detach(), nablas.detach(), [_clone(p.grad) for p in m.parameters()], x.grad.clone(), type(y.grad_fn).__name__
    yf, nf, gf, xf, fn = run()
    assert "FusedMLPFunction" in fn
    # first order: the fused kernel's
    x = x0.clone().requires_grad_(True)
    first, = torch.autograd.grad(m(x)[:, 0].sum(), x)
    gy = torch.zeros(513, 3, device=dev)
    gy[:, 0] = 1.0
    packed = _mlp.pack(desc, [l.weight for l in m.layers], [l.bias for l in m.layers], with_backward=True)
    assert torch.equal(first, _mlp.backward(desc, x0, gy, packed, need_dx=True)[0])
    torch.testing.assert_close(nf, first, rtol=1e-4, atol=1e-5)
    mlp_mod.USE_FUSED = False
    try:
        yt, nt, gt, xt, fn = run()
        assert "FusedMLP" not in fn
    finally:
        mlp_mod.USE_FUSED = True
    assert float(xt.abs().max()) > 0 and all(torch.isfinite(a).all() for a in gf)
    torch.testing.assert_close(yf, yt, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(nf, nt, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(xf, xt, rtol=1e-3, atol=1e-5)
    for a, b in zip(gf, gt):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_sigmoid_hidden_and_unknown_codes_are_refused(dev):
    from nr3d_lib_amd import _hip as H
    from nr3d_lib_amd.bindings import _mlp
    dims = [32, 64, 3]
    m = _net(dims, True, dev)
    ws, bs = [l.weight for l in m.layers], [l.bias for l in m.layers]
    with pytest.raises(RuntimeError):
        _mlp.pack(_mlp.MLPDesc(dims, _mlp.ACT_SIGMOID, _mlp.ACT_NONE), ws, bs)
    with pytest.raises(RuntimeError):
        _mlp.pack_half(_mlp.MLPDesc(dims, _mlp.ACT_SIGMOID, _mlp.ACT_SIGMOID), ws, bs)
    # the C entries themselves, with code 4 in either field and buffers of the sizes the ReLU desc asks for
    good = _mlp.MLPDesc(dims, _mlp.ACT_RELU, _mlp.ACT_SIGMOID)
    n, lib, st = 33, H.lib(), H.stream_of(ws[0])
    for half in (False, True):
        dt = torch.float16 if half else torch.float32
        pre = "nr3d_mlp_half_" if half else "nr3d_mlp_"
        nbytes = (good.half_packed_bytes + good.half_backward_bytes) if half else 4 * (good.packed_floats + good.backward_floats)
        packed = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        wh, bh = [w.detach().to(dt).contiguous() for w in ws], [b.detach().to(dt).contiguous() for b in bs]
        x, gy = torch.zeros(n, dims[0], dtype=dt, device=dev), torch.zeros(n, dims[-1], dtype=dt, device=dev)
        y, dx = torch.zeros(n, dims[-1], dtype=dt, device=dev), torch.zeros(n, dims[0], dtype=dt, device=dev)
        dWs, dbs = _mlp._grad_pool(good, [True] * len(ws), dev)
        for hidden, out in ((_mlp.ACT_RELU, 4), (4, _mlp.ACT_NONE)):
            bad = _mlp.MLPDesc(dims, hidden, out)
            assert not bad.fusable and not bad.half_fusable
            c = C.byref(bad._c)
            assert getattr(lib, pre + "pack")(c, _mlp._ptr_array(wh), _mlp._ptr_array(bh), H.ptr(packed), 1, st) != 0
            assert getattr(lib, pre + "forward")(c, n, H.ptr(x), dims[0], 1, H.ptr(packed), H.ptr(y), dims[-1], st) != 0
            assert getattr(lib, pre + "backward")(c, n, H.ptr(x), dims[0], 1, H.ptr(gy), dims[-1], H.ptr(packed), H.ptr(dx), dims[0], 1,
                                                 _mlp._ptr_array(dWs), _mlp._ptr_array(dbs), st) != 0
            assert lib.nr3d_last_error()
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0 and float(dx.abs().max()) == 0            # nothing ran
