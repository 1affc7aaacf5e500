"""GPU: softplus hidden layers on the fused MLP kernels (csrc/mlp.hip, csrc/mlp_half.hip, csrc/mlp_act.h through bindings._mlp /
models.blocks.MLP) against torch evaluations in float64 on the tests' own tensors -- torch.nn.functional.softplus(h, beta, 20).

fp32: the yardstick of tests/test_mlp_gpu.py -- the error against fp64 stays within max(1e-5 of the output scale, 4 x the error of
torch's own fp32 evaluation).  Softplus has no kinks, so no row is left out anywhere.  Half: the rounded-contract fp64 reference
(tests/mlp_half_ref.py) at 2^-9 of scale for y, 2^-7 for gradients (4 x that for dW / db when n < 100), and every single row of dL/dx
within 2^-7 (tests/test_mlp_softplus_cpu.py: the reference itself moves no row under one more half rounding)."""
import pytest
import torch

from mlp_half_ref import assert_rows, check_rows_against_twin, double_twin, fill_parameters, half_contract, max_excused

pytestmark = pytest.mark.gpu

BETA = 100.0


def _act(beta=BETA, **kw):
    return dict(type="softplus", beta=beta, **kw)


def _net(dims, bias, dev, seed=0, beta=BETA, dtype=torch.float, act=None):
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(seed)
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=act or _act(beta), output_activation=None, bias=bias,
            dtype=dtype, device=dev)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * (0.4 if p.dim() > 1 else 0.2))
    return m


def _activate(layer, h):
    a = layer.activation
    return h if a is None else torch.nn.functional.softplus(h, a.beta, a.threshold)


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
    # dims, n, bias
    ([35, 64, 1], 4099, True),                 # the LoTD SDF decoder of the reference (D = 1, W = 64)
    ([32, 64, 64, 16], 1031, True),
    ([3, 8, 1], 1, True),
    ([16, 32, 32, 32, 7], 513, False),
    ([35, 40, 1], 257, False),                 # padded hidden lanes hold exactly ln 2 / beta (no bias): nothing may read them
]


@pytest.mark.parametrize("dims,n,bias", CASES)
def test_softplus_block_matches_torch(dev, dims, n, bias):
    from nr3d_lib_amd.bindings import _mlp
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net(dims, bias, dev)
    desc = m.fused_desc()
    assert desc is not None and desc.hidden_activation == _mlp.ACT_SOFTPLUS and desc.beta == BETA and desc.backward_fusable
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


def test_three_tile_widths_run_the_forward(dev, hip_option):
    """96-wide hidden layers: the 3-tile class on the 4-tile instantiation -- a whole padded tile of ln 2 / beta per layer; forward only
    (the fused backward stops at 64), both MFMA routes"""
    m = _net([32, 96, 96, 4], True, dev, seed=2)
    desc = m.fused_desc()
    assert desc is not None and desc.fusable and not desc.backward_fusable
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(257, 32, generator=g).to(dev)
    gy = torch.zeros(257, 4, device=dev)
    r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
    for x3 in (1, 0):
        hip_option("mlp_x3", x3)
        with torch.no_grad():
            _check(f"y x3={x3}", m(x), r64[0], r32[0])
    assert "FusedMLP" not in type(m(x).grad_fn).__name__            # gradients wanted: the torch path


def test_which_softplus_fuses(dev):
    """beta = 5 (FUSED_SOFTPLUS_MIN_BETA) runs on the kernels; beta = 1 and threshold = 10 do not, and still give torch's values"""
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(257, 32, generator=g).to(dev)
    gy = torch.randn(257, 16, generator=g).to(dev)
    for act, fused in ((_act(5.0), True), (_act(1.0), False), (_act(100.0, threshold=10), False)):
        m = _net([32, 64, 16], True, dev, seed=4, act=act)
        assert (m.fused_desc() is not None) == fused, act
        x = x0.clone().requires_grad_(True)
        r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
        y = m(x)
        assert tuple(y.shape) == (257, 16) and ("FusedMLPFunction" in type(y.grad_fn).__name__) == fused, act
        y.backward(gy)
        _check_all(str(act), m, y.detach(), x.grad, [l.weight.grad for l in m.layers], [l.bias.grad for l in m.layers], r64, r32)


# ------------------------------------------------------------------------------------------------------------------------
# fp32, every entry of the backward table (csrc/mlp.hip BWD_CASE over NR3D_MLP_BWD_SHAPES x FAST x the bf16 route, SP = true) and the
# forward's XF / X3 selection with the same inputs
# ------------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (1, 2, 1, 1), (1, 2, 1, 2), (1, 2, 2, 1), (1, 2, 2, 2),
              (2, 2, 1, 1), (2, 2, 1, 2), (2, 2, 2, 1), (2, 2, 2, 2)]             # (in, width, out) tiles, hidden layers
TABLE_NS = (257, 1)


def _table_dims(shape, fast):
    """fast 0: ragged widths (dL/dy rows of 3 / 33 elements have no aligned pieces); 1, 2: whole tiles"""
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
def test_every_fp32_backward_table_entry_with_softplus(dev, hip_option, shape, fast, x3):
    from nr3d_lib_amd.bindings import _mlp
    hip_option("mlp_x3", x3)
    dims = _table_dims(shape, fast)
    m = _net(dims, True, dev, seed=21)
    desc = m.fused_desc()
    assert desc is not None and desc.hidden_activation == _mlp.ACT_SOFTPLUS and desc.backward_fusable
    packed = _mlp.pack(desc, [l.weight for l in m.layers], [l.bias for l in m.layers], with_backward=True)
    for n in TABLE_NS:
        x, gy = _table_inputs(dims, n, fast, dev)
        r64, r32 = _table_reference((shape, fast, n), m, x, gy)
        y = _mlp.forward(desc, x, packed)
        dx, dWs, dbs = _mlp.backward(desc, x, gy, packed, need_dx=True)
        assert n == 1 or fast != 2 or dx.stride() == (1, n)
        _check_all(f"n={n}", m, y, dx, dWs, dbs, r64, r32)


# ------------------------------------------------------------------------------------------------------------------------
# fp32, the bf16 three-piece route against the f32 MFMA (form and constants of tests/test_mlp_gpu.py's two ..._is_fp32_grade tests)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [[32, 64, 64, 16], [40, 64, 7]])
def test_softplus_forward_on_the_bf16_mfma_is_fp32_grade(dev, hip_option, dims):
    m = _net(dims, True, dev, seed=13)
    g = torch.Generator(device="cpu").manual_seed(7)
    x = (torch.randn(4099, dims[0], generator=g) * torch.logspace(-3, 3, dims[0])[None, :].clamp(1e-2, 30)).to(dev)    # columns of very different scale
    with torch.no_grad():
        ref = x.double()
        for l in m.layers:
            ref = _activate(l, torch.nn.functional.linear(ref, l.weight.double(), l.bias.double()))
    scale = float(ref.abs().max())
    err = {}
    for mode in (0, 1):
        hip_option("mlp_x3", mode)
        with torch.no_grad():
            y = m(x)
        assert torch.isfinite(y).all()
        err[mode] = float((y.double() - ref).abs().max()) / scale
    print(err)
    assert err[0] < 5e-6 and err[1] < 5e-6, err
    assert err[1] <= 3.0 * err[0] + 2e-7, f"three-piece bf16 route {err[1]:.2e} against the f32 MFMA's {err[0]:.2e}"


@pytest.mark.parametrize("dims", [[32, 64, 64, 16], [40, 64, 7]])
def test_softplus_backward_on_the_bf16_mfma_is_fp32_grade(dev, hip_option, dims):
    m = _net(dims, True, dev, seed=17)
    desc = m.fused_desc()
    assert desc is not None and desc.backward_fusable
    g = torch.Generator(device="cpu").manual_seed(11)
    n = 8205
    x = (torch.randn(n, dims[0], generator=g) * torch.logspace(-2, 1, dims[0])[None, :]).to(dev)
    gy = torch.randn(n, dims[-1], generator=g).to(dev)
    m64 = [(l.weight.detach().double().requires_grad_(True), l.bias.detach().double().requires_grad_(True)) for l in m.layers]
    x64 = x.double().requires_grad_(True)
    h = x64
    for l, (w, b) in zip(m.layers, m64):
        h = _activate(l, torch.nn.functional.linear(h, w, b))
    h.backward(gy.double())
    ref = [x64.grad] + [w.grad for w, _ in m64] + [b.grad for _, b in m64]
    err = {}
    for mode in (0, 1):
        hip_option("mlp_x3", mode)
        xr = x.detach().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        m(xr).backward(gy)
        got = [xr.grad] + [l.weight.grad for l in m.layers] + [l.bias.grad for l in m.layers]
        assert all(torch.isfinite(t).all() for t in got)
        err[mode] = [float((a.double() - b).norm() / b.norm().clamp_min(1e-30)) for a, b in zip(got, ref)]
    print(err)
    assert max(err[0]) < 2e-5 and max(err[1]) < 2e-5, err
    for e0, e1 in zip(err[0], err[1]):
        assert e1 <= 3.0 * e0 + 1e-6, f"three-piece bf16 backward {e1:.2e} against the f32 MFMA's {e0:.2e}"


# ------------------------------------------------------------------------------------------------------------------------
# fp32: saturation, layouts, forward_columns
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [0, 1])
def test_saturated_units_stay_finite(dev, hip_option, x3):
    """x scaled until pre-activations pass +-100, i.e. beta z = +-1e4: exp overflows on one side and vanishes on the other -- h = z /
    h = 0 and derivative 1 / 0 without an inf * 0; y and every gradient finite and equal to fp64's"""
    hip_option("mlp_x3", x3)
    dims = [32, 64, 64, 16]
    m = _net(dims, True, dev, seed=31)
    g = torch.Generator(device="cpu").manual_seed(32)
    x = (torch.randn(1031, 32, generator=g) * 40.0).to(dev).requires_grad_(True)
    gy = torch.randn(1031, 16, generator=g).to(dev)
    with torch.no_grad():
        z1 = torch.nn.functional.linear(x.double(), m.layers[0].weight.double(), m.layers[0].bias.double())
        assert float(z1.max()) > 100.0 and float(z1.min()) < -100.0
    r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
    y = m(x)
    y.backward(gy)
    _check_all(f"x3={x3}", m, y.detach(), x.grad, [l.weight.grad for l in m.layers], [l.bias.grad for l in m.layers], r64, r32)


def test_feature_major_input_is_consumed_in_place(dev):
    from nr3d_lib_amd.bindings import _mlp
    dims, n = [32, 64, 1], 257
    m = _net(dims, True, dev, seed=3)
    g = torch.Generator(device="cpu").manual_seed(4)
    xt = torch.randn(dims[0], n, generator=g).to(dev).requires_grad_(True)
    x = xt.t()
    assert x.stride() == (1, n)
    gy = torch.randn(n, 1, generator=g).to(dev)
    r64, r32 = _reference(m, x, gy, torch.float64), _reference(m, x, gy, torch.float32)
    y = m(x)
    y.backward(gy)
    _check_all("module", m, y.detach(), xt.grad.t(), [l.weight.grad for l in m.layers], [l.bias.grad for l in m.layers], r64, r32)
    desc = m.fused_desc()
    packed = _mlp.pack(desc, [l.weight for l in m.layers], [l.bias for l in m.layers], with_backward=True)
    dx, dWs, dbs = _mlp.backward(desc, x.detach(), gy, packed, need_dx=True)
    assert dx.stride() == (1, n)
    _check_all("binding", m, _mlp.forward(desc, x.detach(), packed), dx, dWs, dbs, r64, r32)


@pytest.mark.parametrize("dtype", [torch.float, torch.half])
def test_forward_columns_carries_beta(dev, hip_option, dtype):
    """forward_columns builds a sub-desc: with beta carried over, its column is the sliced full forward bit for bit"""
    m = _net([32, 64, 16], True, dev, seed=5, dtype=dtype)
    assert m.fused_desc() is not None
    x = torch.randn(1031, 32, device=dev).to(dtype)
    for x3 in ((1, 0) if dtype == torch.float else (1,)):
        hip_option("mlp_x3", x3)
        with torch.no_grad():
            full = m(x)
            part = m.forward_columns(x, 1)
        assert tuple(part.shape) == (1031, 1) and part.dtype == full.dtype and torch.isfinite(full).all()
        assert torch.equal(part, full[:, :1]), f"x3={x3}"


# ------------------------------------------------------------------------------------------------------------------------
# second order: no fused double backward for softplus -- the create_graph backward differentiates the torch evaluation
# ------------------------------------------------------------------------------------------------------------------------
def _clone(g):
    """a parameter's gradient as an fp32 copy; None stays None (the output layer's bias does not reach the nablas)"""
    return None if g is None else g.float().clone()


def _hidden_biases_got_a_gradient(m, grads):
    last = f"layers.{len(m.layers) - 1}."
    for (name, _), ga in zip(m.named_parameters(), grads):
        assert ga is None or torch.isfinite(ga).all(), name
        if name.endswith("bias") and not name.startswith(last):
            assert ga is not None and float(ga.abs().max()) > 0, f"{name}: the eikonal term gives the hidden biases a gradient"


def _eikonal_run(m, x0, dt=torch.float32):
    m.zero_grad(set_to_none=True)
    x = x0.to(dt).clone().requires_grad_(True)
    y = m(x)
    nablas, = torch.autograd.grad((y[:, 0] if dt == torch.float64 else y[:, 0].float()).sum(), x, create_graph=True)
    assert nablas.requires_grad
    return x, y, nablas


def test_second_order_through_the_softplus_block(dev):
    """the eikonal pattern of test_second_order_through_the_fused_block on a softplus network: fused block against USE_FUSED = False
    at that test's tolerances; and, softplus not being piecewise linear, the eikonal term ALONE gives x and the biases a gradient"""
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    m = _net([16, 32, 32, 4], True, dev, seed=5)
    assert m.fused_desc() is not None and not m.fused_desc().second_order_fusable
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(513, 16, generator=g).to(dev)

    def run(eik_only=False):
        x, y, nablas = _eikonal_run(m, x0)
        eik = ((nablas.norm(dim=-1) - 1.0) ** 2).mean()
        (eik if eik_only else eik + y.square().mean()).backward()
        return y.detach(), nablas.detach(), [_clone(p.grad) for p in m.parameters()], x.grad.clone(), type(y.grad_fn).__name__
    yf, nf, gf, xf, fn = run()
    assert "FusedMLPFunction" in fn
    _, _, ge, xe, _ = run(eik_only=True)
    assert torch.isfinite(xe).all() and float(xe.abs().max()) > 0, "the eikonal term gives x a gradient"
    _hidden_biases_got_a_gradient(m, ge)
    mlp_mod.USE_FUSED = False
    try:
        yt, nt, gt, xt, fn = run()
        assert "FusedMLP" not in fn
    finally:
        mlp_mod.USE_FUSED = True
    torch.testing.assert_close(yf, yt, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(nf, nt, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(xf, xt, rtol=1e-3, atol=1e-5)
    for a, b in zip(gf, gt):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-5)


def test_second_order_through_the_half_softplus_block(dev):
    """the same through MLP(dtype=half): fused half block against USE_FUSED = False (the autocast layers), whose second order both
    evaluate in fp32 from the fp32 parameters.  Softplus has no kink, so EVERY row of the nablas and of x.grad is held
    (tests/mlp_half_ref.py check_rows_against_twin) to max(2e-2, 4 x the USE_FUSED = False run's worst row) of the tensor's scale
    against an fp64 twin of the module: parameters and x rounded to half, everything else double.  The earlier comparison with the
    USE_FUSED = False run itself stays beside it.  Measured on an MI355X, worst row as a fraction of scale, fused (USE_FUSED = False):
    nablas 1.9e-3 (7.2e-4), x.grad 6.3e-3 (1.5e-3) -- 2e-2 is the bound in force."""
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    torch.manual_seed(11)
    m = MLP(16, 4, D=2, W=32, activation=_act(), dtype=torch.half, device=torch.device("cpu")).to(dev)      # drawn on the CPU
    twin = double_twin(m)
    assert m.fused_desc() is not None and m.fused_desc().half_backward_fusable
    g = torch.Generator(device="cpu").manual_seed(4)
    x0 = torch.randn(513, 16, generator=g).to(dev)

    def run(eik_only=False):
        x, y, nablas = _eikonal_run(m, x0)
        eik = ((nablas.float().norm(dim=-1) - 1.0) ** 2).sum()
        (eik if eik_only else eik + y.float().square().sum()).backward()
        return nablas.detach().float(), [_clone(p.grad) for p in m.parameters()], x.grad.float().clone(), type(y.grad_fn).__name__

    def run64():
        x, y, nablas = _eikonal_run(twin, x0.half(), torch.float64)
        (((nablas.norm(dim=-1) - 1.0) ** 2).sum() + y.square().sum()).backward()
        return nablas.detach(), x.grad.clone()
    nh, gh, xh, fn = run()
    assert "FusedMLPHalfFunction" in fn
    _, ge, xe, _ = run(eik_only=True)
    assert torch.isfinite(xe).all() and float(xe.abs().max()) > 0
    _hidden_biases_got_a_gradient(m, ge)
    mlp_mod.USE_FUSED = False
    try:
        nr, gr, xr, fn = run()
        assert "FusedMLP" not in fn
    finally:
        mlp_mod.USE_FUSED = True

    def rows_off(a, b, tol=2e-2):
        return float(((a - b).abs().amax(1) > tol * float(b.abs().max())).float().mean())
    assert torch.isfinite(nh).all() and torch.isfinite(xh).all()
    n64, x64 = run64()
    check_rows_against_twin("nablas", nh, nr, n64)
    check_rows_against_twin("x.grad", xh, xr, x64)
    assert rows_off(nh, nr) < 0.05, f"nablas: {rows_off(nh, nr):.3f} of the rows differ"
    assert rows_off(xh, xr) < 0.05, f"x.grad: {rows_off(xh, xr):.3f} of the rows differ"
    for i, (a, b) in enumerate(zip(gh, gr)):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, f"param {i}"
        err = float((a - b).norm() / b.norm())
        assert err < 5e-2, f"param {i}: relative difference of the gradient {err:.3e}"


# ------------------------------------------------------------------------------------------------------------------------
# half precision on the f16 MFMA (csrc/mlp_half.hip): MLP(dtype=torch.half) with softplus hidden layers
# ------------------------------------------------------------------------------------------------------------------------
HALF_DIMS = [[35, 64, 1], [32, 64, 64, 16], [32, 32, 32, 32, 16]]      # k_mlph_bwd_split (one and two 64-wide layers), k_mlph_bwd (three 32-wide)
HALF_NS = (1031, 33)


def half_net(dims, dev):
    from nr3d_lib_amd.models.blocks import MLP
    torch.manual_seed(0)
    m = MLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=_act(), bias=True, dtype=torch.half, device=dev)
    return fill_parameters(m, 0)                    # from a CPU generator: the CPU tests see the same nets


def half_inputs(dims, n, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    return torch.randn(n, dims[0], generator=g).to(dev), torch.randn(n, dims[-1], generator=g).to(dev)


def _check_half(name, got, ref64, tol):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64).abs().max()) / scale
    print(f"{name}: rel err {err:.2e} (tol {tol:.2e})")
    assert torch.isfinite(got).all() and err <= tol, f"{name}: rel err {err:.2e} > {tol:.2e}"


@pytest.mark.parametrize("layout", ["row_major", "feature_major"])
@pytest.mark.parametrize("n", HALF_NS)
@pytest.mark.parametrize("dims", HALF_DIMS)
def test_half_softplus_forward_backward(dev, dims, n, layout):
    m = half_net(dims, dev)
    desc = m.fused_desc()
    assert desc is not None and desc.half_fusable and desc.half_backward_fusable
    xs, gy = half_inputs(dims, n, dev)
    if layout == "feature_major":
        xt = xs.t().contiguous().requires_grad_(True)
        x = xt.t()
    else:
        xt = x = xs.clone().requires_grad_(True)
    contract = half_contract(m, x, gy)
    y64, dx64, dW64, db64, zs = contract
    assert not zs                                   # no ReLU layer: assert_rows excuses no row
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
