"""GPU: the Lipschitz weight normalisation (csrc/mlp_lipschitz.hip k_lipschitz_normalize / k_lipschitz_normalize_bwd through
bindings._mlp.lipschitz_normalize[_backward]) and ``LipshitzMLP`` on top of it (models.blocks.mlp, ``FUSED_LIPSHITZ``).

* On the lattice of tests/mlp_lipschitz_ref.py every intermediate is exact in float32 in any summation order: W~, dL/dW and dL/dc must
  EQUAL the float64 restatement, for float and half weights, all seven shapes in one call and split 1 + 6, and two calls must give
  the same bytes.
* Off the lattice: W~ within (cols + 8) 2^-24 relative of the float64 restatement of the same float32 inputs (worst-case float32
  summation of cols non-negative terms, one division, one product, a softplus of a few ulp; the accuracy of expf / log1pf on the device
  is taken from HIP's documentation); half weights within one half ulp-spacing.  Gradients: the error against float64 is at most 8 x
  the error of torch's own fp32 chain on the same inputs and device -- the factor tests/test_mlp_softplus_second_order_gpu.py allows the
  fused decoder.  torch's own error on a tensor of seven numbers (dL/dc) or on a 1 x 1 layer can be 0 by luck, so there is a floor:
  2^-20 = 16 float32 roundings of the magnitude of the terms (_gradient_scales) -- the depth of the kernel's own arithmetic at these
  shapes: at most 5 sequential additions per lane (257 columns over 64 lanes), 6 levels of the wave's tree, one rounding per product, and
  the division and two products behind the sums.  Every check prints its figures ("YARDSTICK ..."; profiles/mlp_lipschitz.json keeps one run).
* Non-finite rows (a NaN, a +Inf, an all-zero row, c = -200 whose softplus underflows to 0) give what the torch chain gives on the same
  device, NaN equal to NaN.
* End to end: fused route against the unfused route of the same module (and float64), with the yardsticks of the plain MLP's tests
  (tests/test_mlp_sigmoid_gpu.py: 4 x torch's error, half 2^-8 / 2^-6; tests/test_mlp_softplus_second_order_gpu.py: 8 x for the eikonal
  step); the fused decoder functions must really be taken, and no stale packed buffer may survive a step on c."""
import contextlib

import numpy as np
import pytest
import torch

import mlp_lipschitz_ref as R

pytestmark = pytest.mark.gpu

SOFTPLUS = dict(type="softplus", beta=100.0)


@contextlib.contextmanager
def _switch(**names):
    """module switches of models.blocks.mlp for the block, restored afterwards"""
    from nr3d_lib_amd.models.blocks import mlp as mlp_mod
    saved = {k: getattr(mlp_mod, k) for k in names}
    try:
        for k, val in names.items():
            setattr(mlp_mod, k, val)
        yield mlp_mod
    finally:
        for k, val in saved.items():
            setattr(mlp_mod, k, val)


@contextlib.contextmanager
def _spy(name):
    """count the calls of bindings._mlp.<name>"""
    from nr3d_lib_amd.bindings import _mlp
    real, calls = getattr(_mlp, name), []

    def wrapped(*a, **kw):
        calls.append(name)
        return real(*a, **kw)

    setattr(_mlp, name, wrapped)
    try:
        yield calls
    finally:
        setattr(_mlp, name, real)


# ------------------------------------------------------------------------------------------------------------------------
# the kernels on the lattice: exact
# ------------------------------------------------------------------------------------------------------------------------
_lattice = {}


def lattice():
    """the lattice network and its restatement, computed once"""
    if not _lattice:
        Ws, Gs, c = R.lattice_network(seed=7)
        _lattice["in"] = (Ws, Gs, c)
        _lattice["fwd"] = [R.normalize(W, cl) for W, cl in zip(Ws, c)]
        _lattice["bwd"] = [R.normalize_backward(W, cl, G) for W, cl, G in zip(Ws, c, Gs)]
    return _lattice


def _bits(t):
    """the tensor's bytes as integers (a NaN equals itself)"""
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _run(dev, Ws, Gs, c, half, groups):
    """the binding on the layers [lo, hi) of every group -> ([W~], [dW], dc) as numpy, layers in order"""
    from nr3d_lib_amd.bindings import _mlp
    dt = torch.float16 if half else torch.float32
    wt, dw, dc = [], [], []
    for lo, hi in groups:
        ws = [torch.from_numpy(W).to(dev).to(dt) for W in Ws[lo:hi]]
        gs = [torch.from_numpy(G).to(dev) for G in Gs[lo:hi]]
        ct = torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev)
        out = _mlp.lipschitz_normalize(ws, ct)
        assert all(o.dtype == dt and o.shape == w.shape for o, w in zip(out, ws))
        g_w, g_c = _mlp.lipschitz_normalize_backward(ws, ct, gs)
        assert all(g.dtype == torch.float32 and g.shape == w.shape for g, w in zip(g_w, ws)) and tuple(g_c.shape) == (hi - lo,)
        # the same inputs give the same bytes
        out2 = _mlp.lipschitz_normalize(ws, ct)
        g_w2, g_c2 = _mlp.lipschitz_normalize_backward(ws, ct, gs)
        for a, b in zip([*out, *g_w, g_c], [*out2, *g_w2, g_c2]):
            assert torch.equal(_bits(a), _bits(b))
        wt += [o.cpu().numpy() for o in out]
        dw += [g.cpu().numpy() for g in g_w]
        dc += g_c.cpu().tolist()
    return wt, dw, np.array(dc)


@pytest.mark.parametrize("groups", [((0, 7),), ((0, 1), (1, 7))], ids=["7", "1+6"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_kernels_equal_the_restatement_on_the_lattice(dev, half, groups):
    L = lattice()
    Ws, Gs, c = L["in"]
    assert tuple(W.shape for W in Ws) == R.LATTICE_SHAPES
    wt, dw, dc = _run(dev, Ws, Gs, c, half, groups)
    for l, shape in enumerate(R.LATTICE_SHAPES):
        assert np.array_equal(wt[l].astype(np.float64), L["fwd"][l]), f"W~ of layer {l} {shape}"
        assert np.array_equal(dw[l].astype(np.float64), L["bwd"][l][0]), f"dL/dW of layer {l} {shape}"
        assert float(dc[l]) == L["bwd"][l][1], f"dL/dc of layer {l} {shape}: {dc[l]} != {L['bwd'][l][1]}"
    # every kind of row took part: clamped (W~ == W), tie, scaled, zero
    a = np.concatenate([np.abs(W.astype(np.float64)).sum(1) for W in Ws])
    assert set(a) == set(R.ABS_SUMS)


# ------------------------------------------------------------------------------------------------------------------------
# off the lattice
# ------------------------------------------------------------------------------------------------------------------------
def _inverse_softplus(sp):
    return float(sp) if sp > 20 else float(np.log(np.expm1(sp)))


def random_network(half, seed=11):
    """random weights in the lattice's shapes, c_l such that softplus(c_l) separates the lower half of the row abs-sums from the upper
    half (midway between two of them: no row sits at the tie); one row only: scaled"""
    rng = np.random.default_rng(seed)
    Ws, Gs, c = [], [], []
    for rows, cols in R.LATTICE_SHAPES:
        W = (rng.standard_normal((rows, cols)) * 0.4).astype(np.float16 if half else np.float32).astype(np.float32)
        a = np.sort(np.abs(W.astype(np.float64)).sum(1))
        sp = 0.75 * a[0] if rows == 1 else 0.5 * (a[rows // 2 - 1] + a[rows // 2])
        Ws.append(W)
        Gs.append(rng.standard_normal((rows, cols)).astype(np.float32))
        c.append(_inverse_softplus(sp))
    return Ws, Gs, np.array(c, np.float32)


def _gradient_scales(W, c, G):
    """the magnitudes the gradients' rounding errors are relative to (float64): dL/dW is a DIFFERENCE of G q and sign(W) S q / den, and
    S and dL/dc are sums with cancellation (a 1 x 1 layer's dL/dW is exactly 0 where the row is scaled), so the scale is that of the
    terms, sum_j |G W| in place of S: (max |G q| + max_r sum_j |G W| q / den, softplus'(c) sum_r sum_j |G W| / den)"""
    W, G = W.astype(np.float64), G.astype(np.float64)
    sp = R.softplus(c)
    den = np.maximum(np.abs(W).sum(1), sp)
    s_abs = np.abs(G * W).sum(1)
    return float(np.abs(G * (sp / den)[:, None]).max() + (s_abs * sp / den ** 2).max()), float(R.sigmoid(c) * (s_abs / den).sum())


def _yardstick(name, got, ref64, ref32, scale, factor=8.0, floor=2.0 ** -20):
    err = float((np.abs(got.astype(np.float64) - ref64) / scale).max())
    err32 = float((np.abs(ref32.astype(np.float64) - ref64) / scale).max())
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert np.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(floor, factor * err32), f"{name}: rel err {err:.2e} (torch fp32 chain: {err32:.2e})"


def _torch_chain(dev, Ws, Gs, c):
    """the reference's expression and its autograd in fp32 on the device -> ([W~], [dW], dc) as numpy"""
    from nr3d_lib_amd.models.blocks import LipshitzMLP
    m = LipshitzMLP(3, 3, D=1, W=4)
    ct = torch.from_numpy(c).to(dev).requires_grad_(True)
    wt, dw = [], []
    for l, (W, G) in enumerate(zip(Ws, Gs)):
        w = torch.from_numpy(W).to(dev).requires_grad_(True)
        out = m.normalization(w, torch.nn.functional.softplus(ct[l]))
        out.backward(torch.from_numpy(G).to(dev))
        wt.append(out.detach().cpu().numpy())
        dw.append(w.grad.cpu().numpy())
    return wt, dw, ct.grad.cpu().numpy()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_random_weights_against_float64(dev, half):
    Ws, Gs, c = random_network(half)
    wt, dw, dc = _run(dev, Ws, Gs, c, half, ((0, 7),))
    t_wt, t_dw, t_dc = _torch_chain(dev, Ws, Gs, c)
    scaled = total = 0
    for l, (W, G) in enumerate(zip(Ws, Gs)):
        rows, cols = W.shape
        ref = R.normalize(W, c[l])
        err = np.abs(wt[l].astype(np.float64) - ref)
        if half:
            tol = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)
        else:
            tol = (cols + 8) * 2.0 ** -24 * np.abs(ref)
        worst = float((err / np.where(tol > 0, tol, 1.0)).max())
        print(f"YARDSTICK W~[{l}] {rows}x{cols} {'half' if half else 'fp32'}: largest error / bound {worst:.3f}")
        assert np.isfinite(wt[l]).all() and (err <= tol).all(), f"W~ of layer {l}: {worst:.2f} x the bound"
        a = np.abs(W.astype(np.float64)).sum(1)
        scaled += int((a > R.softplus(c[l])).sum())
        total += rows
        # clamped rows pass through bit for bit
        keep = a < R.softplus(c[l]) * (1 - 1e-6)
        assert np.array_equal(wt[l][keep].astype(np.float32), W[keep])
    assert 0.4 * total <= scaled <= 0.6 * total
    ref_dc, scale_dc = [], []
    for l, (W, G) in enumerate(zip(Ws, Gs)):
        ref_dw, d = R.normalize_backward(W, c[l], G)
        scale_dw, s = _gradient_scales(W, c[l], G)
        ref_dc.append(d)
        scale_dc.append(s)
        _yardstick(f"dL/dW[{l}] {W.shape[0]}x{W.shape[1]} {'half' if half else 'fp32'}", dw[l], ref_dw, t_dw[l], scale_dw)
    _yardstick(f"dL/dc {'half' if half else 'fp32'}", dc, np.array(ref_dc), t_dc, np.array(scale_dc))


# ------------------------------------------------------------------------------------------------------------------------
# non-finite rows
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_non_finite_rows_as_the_torch_chain(dev, half):
    """lattice layers (exact sums: the finite rows do not depend on torch's summation order) with a NaN, a +Inf and the lattice's all-zero
    row in layer 0, and a layer whose c = -200: softplus underflows to 0, its rows scale to 0 and its zero row is 0 / 0"""
    Ws, Gs, c = R.lattice_network(seed=3, shapes=((8, 35), (7, 64), (6, 3)))
    Ws[0][0, 4] = np.nan
    Ws[0][1, 9] = np.inf
    assert not Ws[0][5].any() and not Ws[2][5].any()
    c[2] = -200.0
    wt, dw, dc = _run(dev, Ws, Gs, c, half, ((0, 3),))
    t_wt, t_dw, t_dc = _torch_chain(dev, Ws, Gs, c)
    for l in range(3):
        want = torch.from_numpy(t_wt[l]).half().numpy() if half else t_wt[l]
        assert np.array_equal(wt[l], want, equal_nan=True), f"W~ of layer {l}"
        assert np.array_equal(dw[l], t_dw[l], equal_nan=True), f"dL/dW of layer {l}"
    assert np.array_equal(dc, t_dc, equal_nan=True), (dc, t_dc)
    # what the rows are: NaN row all NaN; Inf row NaN at the Inf, 0 elsewhere; zero row 0; c = -200: 0, its zero row NaN
    assert np.isnan(wt[0][0]).all() and np.isnan(wt[0][1, 9]) and not np.delete(wt[0][1], 9).any() and not wt[0][5].any()
    assert np.isfinite(wt[0][2:]).all() and np.isfinite(wt[1]).all() and np.isfinite(dw[1]).all() and np.isfinite(dc[1])
    assert not wt[2][:5].any() and np.isnan(wt[2][5]).all() and np.isnan(dc[0]) and np.isnan(dc[2])


# ------------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------------
def _net(dims, dev, hidden="relu", out="sigmoid", dtype=torch.float, seed=0, bound_factor=0.5):
    """LipshitzMLP with the 0.4 / 0.2 randn parameters of the fused MLP tests (0.1 in front of a sigmoid), the bounds at
    ``bound_factor`` x the inf-norms: rows are scaled"""
    from nr3d_lib_amd.models.blocks import LipshitzMLP
    torch.manual_seed(seed)
    m = LipshitzMLP(dims[0], dims[-1], D=len(dims) - 2, W=dims[1:-1], activation=hidden, output_activation=out, dtype=dtype, device=dev)
    with torch.no_grad():
        for layer in m.layers:
            layer.weight.copy_(torch.randn_like(layer.weight) * 0.4)
            layer.bias.copy_(torch.randn_like(layer.bias) * 0.2)
        if out == "sigmoid":
            m.layers[-1].weight.mul_(0.25)
        m.lipshitz_bound_per_layer.copy_(m.initial_bounds(bound_factor))
        sp = torch.nn.functional.softplus(m.lipshitz_bound_per_layer)
        n_scaled = sum(int((l.weight.abs().sum(1) > s).sum()) for l, s in zip(m.layers, sp))
    assert n_scaled >= len(m.layers)
    return m


def _double_twin(m, dims, dev, hidden, out):
    m64 = _net(dims, dev, hidden, out).double()
    m64.load_state_dict({k: val.double() for k, val in m.state_dict().items()})
    return m64


def _step(m, x0, gy, dt=torch.float32):
    """forward + backward -> (y, x.grad, {name: grad}, grad_fn name)"""
    m.zero_grad(set_to_none=True)
    x = x0.to(dt).clone().requires_grad_(True)
    y = m(x)
    y.backward(gy.to(y.dtype))
    return y.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, type(y.grad_fn).__name__


def _check(name, got, ref64, ref32, factor):
    """the yardstick of tests/test_mlp_sigmoid_gpu.py (factor 4) / tests/test_mlp_softplus_second_order_gpu.py (factor 8)"""
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64.double()).abs().max()) / scale
    err32 = float((ref32.double() - ref64.double()).abs().max()) / scale
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(1e-5, factor * err32), f"{name}: rel err {err:.2e} (torch fp32 path: {err32:.2e})"


def _inputs(dims, n, dev, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, dims[0], generator=g).to(dev), torch.randn(n, dims[-1], generator=g).to(dev)


def test_fp32_block_on_the_fused_decoder(dev):
    dims, n = [35, 64, 64, 3], 300
    m = _net(dims, dev)
    x0, gy = _inputs(dims, n, dev)
    with _switch(FUSED_LIPSHITZ=True), _spy("lipschitz_normalize") as fwd, _spy("lipschitz_normalize_backward") as bwd, \
            _spy("forward") as dec_f, _spy("backward") as dec_b:
        yf, xf, gf, fn = _step(m, x0, gy)
        assert fn == "FusedMLPFunctionBackward" and len(fwd) == 1 and len(bwd) == 1 and len(dec_f) == 1 and len(dec_b) == 1
        with torch.no_grad():
            assert torch.equal(m(x0), yf)
    with _switch(FUSED_LIPSHITZ=False), _spy("lipschitz_normalize") as fwd, _spy("forward") as dec_f:
        yt, xt, gt, fn = _step(m, x0, gy)
        assert "FusedMLP" not in fn and not fwd and not dec_f
        y64, x64, g64, _ = _step(_double_twin(m, dims, dev, "relu", "sigmoid"), x0, gy, torch.float64)
    _check("fp32 y", yf, y64, yt, 4)
    _check("fp32 dL/dx", xf, x64, xt, 4)
    assert set(gf) == set(gt) and "lipshitz_bound_per_layer" in gf
    for k in gf:
        _check(f"fp32 dL/d {k}", gf[k], g64[k], gt[k], 4)
    assert float(gf["lipshitz_bound_per_layer"].abs().min()) > 0


def test_half_block_on_the_fused_decoder(dev):
    """the bounds of test_half_sigmoid_agrees_with_the_autocast_layers: y within 2^-8 of scale, parameter gradients (sums over the rows)
    within 2^-6; dL/dx row by row within 2^-6 of scale except at most max(2, n // 2000) rows (a unit within half rounding of its ReLU
    kink flips between the two routes)"""
    dims, n = [35, 64, 64, 3], 300
    m = _net(dims, dev, dtype=torch.half)
    x0, gy = _inputs(dims, n, dev)
    with _switch(FUSED_LIPSHITZ=True), _spy("lipschitz_normalize") as fwd, _spy("forward_half") as dec_f, _spy("backward_half") as dec_b:
        yf, xf, gf, fn = _step(m, x0, gy)
        assert fn == "FusedMLPHalfFunctionBackward" and yf.dtype == torch.float16 and len(fwd) == 1 and len(dec_f) == 1 and len(dec_b) == 1
    with _switch(FUSED_LIPSHITZ=False):
        yt, xt, gt, fn = _step(m, x0, gy)
        assert "FusedMLP" not in fn and yt.dtype == torch.float16
    scale = float(yt.float().abs().max())
    err = float((yf.float() - yt.float()).abs().max())
    print(f"YARDSTICK half y: err / scale {err / scale:.3e} (bound {2.0 ** -8:.3e})")
    assert err <= 2.0 ** -8 * scale
    for k in gf:
        e, s = float((gf[k] - gt[k]).abs().max()), float(gt[k].abs().max())
        print(f"YARDSTICK half dL/d {k}: err / scale {e / s:.3e} (bound {2.0 ** -6:.3e})")
        assert gf[k].dtype == torch.float32 and e <= 2.0 ** -6 * s, k
    bad = int(((xf.float() - xt.float()).abs().amax(1) > 2.0 ** -6 * float(xt.float().abs().max())).sum())
    print(f"YARDSTICK half dL/dx: {bad} of {n} rows beyond 2^-6 of scale")
    assert bad <= 2


def _eikonal_step(m, x0, dt=torch.float32):
    m.zero_grad(set_to_none=True)
    x = x0.to(dt).clone().requires_grad_(True)
    y = m(x)
    nablas, = torch.autograd.grad(y[:, 0].sum(), x, create_graph=True)
    loss = ((nablas.norm(dim=-1) - 1.0) ** 2).mean() + y.square().mean()
    loss.backward()
    return {k: p.grad.clone() for k, p in m.named_parameters()}, x.grad.clone(), nablas.detach(), type(nablas.grad_fn).__name__


def test_eikonal_step_through_the_lipshitz_sdf_decoder(dev):
    dims, n = [35, 64, 1], 300
    m = _net(dims, dev, SOFTPLUS, None, seed=7)
    x0, _ = _inputs(dims, n, dev, seed=5)
    with _switch(FUSED_LIPSHITZ=True, FUSED_SECOND_ORDER=True, FUSED_SOFTPLUS_SECOND_ORDER=True), \
            _spy("backward_backward_softplus") as bb, _spy("lipschitz_normalize_backward") as bwd:
        gf, xf, nf, fn = _eikonal_step(m, x0)
        assert fn == "FusedMLPBackwardFunctionBackward" and len(bb) == 1 and len(bwd) == 1
    with _switch(FUSED_LIPSHITZ=False):
        gt, xt, nt, fn = _eikonal_step(m, x0)
        assert fn != "FusedMLPBackwardFunctionBackward"
        g64, x64, n64, _ = _eikonal_step(_double_twin(m, dims, dev, SOFTPLUS, None), x0, torch.float64)
    _check("eikonal nablas", nf, n64, nt, 8)
    _check("eikonal dL/dx", xf, x64, xt, 8)
    for k in gf:
        _check(f"eikonal dL/d {k}", gf[k], g64[k], gt[k], 8)
    assert float(gf["lipshitz_bound_per_layer"].abs().min()) > 0


@pytest.mark.parametrize("cache", [False, True], ids=["nocache", "CACHE_PACKED"])
@pytest.mark.parametrize("dtype", [torch.float, torch.half], ids=["fp32", "half"])
def test_a_step_on_the_bounds_changes_the_next_forward(dev, dtype, cache):
    """no stale packed buffer: the packed weights of a Lipschitz network depend on (W, b, c)"""
    dims, n = [35, 64, 64, 3], 300
    m = _net(dims, dev, dtype=dtype)
    x0, gy = _inputs(dims, n, dev)
    c = m.lipshitz_bound_per_layer
    tol = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float else dict(rtol=2.0 ** -7, atol=2.0 ** -8)

    def unfused():
        with _switch(FUSED_LIPSHITZ=False), torch.no_grad():
            return m(x0)

    with _switch(FUSED_LIPSHITZ=True, CACHE_PACKED=cache):
        opt = torch.optim.SGD([c], lr=1.0)
        y0 = m(x0)
        assert "FusedMLP" in type(y0.grad_fn).__name__
        y0.backward(gy.to(y0.dtype))
        assert float(c.grad.abs().min()) > 0
        c.grad.copy_(0.25 * c.detach())                       # a step of a known size: c <- 0.75 c
        opt.step()
        y1 = m(x0)
        assert not torch.equal(y1, y0)
        torch.testing.assert_close(y1.detach(), unfused(), **tol)
        # eval / no_grad: computed once and reused (CACHE_PACKED), and dropped by load_state_dict
        m.eval()
        with torch.no_grad(), _spy("lipschitz_normalize") as fwd:
            ya, yb = m(x0), m(x0)
            assert torch.equal(ya, yb) and torch.equal(ya, y1.detach()) and len(fwd) == (1 if cache else 2)
            sd = {k: val.clone() for k, val in m.state_dict().items()}
            sd["lipshitz_bound_per_layer"] *= 0.5
            m.load_state_dict(sd, strict=True)
            yc = m(x0)
            assert not torch.equal(yc, ya)
            torch.testing.assert_close(yc, unfused(), **tol)
            # ... and an in-place edit of c that bumps its version is seen too
            c.mul_(1.5)
            yd = m(x0)
            assert not torch.equal(yd, yc)
            torch.testing.assert_close(yd, unfused(), **tol)


def test_wide_network_normalises_through_the_kernel(dev):
    """W = 256: outside the fused decoder, so the layers run on torch -- on weights from the one-launch normalisation"""
    dims, n = [35, 256, 256, 3], 64
    m = _net(dims, dev)
    assert m.fused_desc() is None
    x0, gy = _inputs(dims, n, dev)
    with _switch(FUSED_LIPSHITZ=True), _spy("lipschitz_normalize") as fwd, _spy("lipschitz_normalize_backward") as bwd, _spy("forward") as dec:
        yf, xf, gf, fn = _step(m, x0, gy)
        assert "FusedMLP" not in fn and len(fwd) == 1 and len(bwd) == 1 and not dec
        y2, last = m(x0, return_last=True)
        assert torch.equal(y2.detach(), yf) and tuple(last.shape) == (n, 256)
    with _switch(FUSED_LIPSHITZ=False), _spy("lipschitz_normalize") as fwd:
        yt, xt, gt, fn = _step(m, x0, gy)
        assert not fwd
        y64, x64, g64, _ = _step(_double_twin(m, dims, dev, "relu", "sigmoid"), x0, gy, torch.float64)
    _check("wide y", yf, y64, yt, 4)
    _check("wide dL/dx", xf, x64, xt, 4)
    for k in gf:
        _check(f"wide dL/d {k}", gf[k], g64[k], gt[k], 4)


def test_return_last_and_cpu_module_keep_the_torch_chain(dev):
    """return_last on a fusable network: the normalisation through the kernel, the layers on torch; a CPU module never reaches a kernel"""
    dims = [35, 64, 64, 3]
    m = _net(dims, dev)
    x0, _ = _inputs(dims, 300, dev)
    with _switch(FUSED_LIPSHITZ=True), _spy("lipschitz_normalize") as fwd, _spy("forward") as dec, torch.no_grad():
        y, last = m(x0, return_last=True)
        assert len(fwd) == 1 and not dec and tuple(last.shape) == (300, 64)
        torch.testing.assert_close(y, m(x0), rtol=1e-4, atol=1e-5)
        from nr3d_lib_amd.models.blocks import LipshitzMLP
        mc = LipshitzMLP(35, 3, D=2, W=64, output_activation="sigmoid")
        mc.load_state_dict({k: val.cpu() for k, val in m.state_dict().items()})
        torch.testing.assert_close(mc(x0.cpu()), y.cpu(), rtol=1e-4, atol=1e-5)
        assert len(fwd) == 2
