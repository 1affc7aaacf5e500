"""GPU: the SH and frequency embedders (csrc/embed.hip) through the C ABI twins and through the modules, against the fp64 restatement
(tests/embedders_ref.py) within bounds derived from the evaluation order, never from the results.

SH bound.  Column c: |got - ref64| <= K * 2^-24 * M_c(x, y, z) (+ 2^-126, the smallest normal, for results that underflow), M_c the
column's polynomial with every coefficient and variable replaced by its absolute value.  K counts the roundings one monomial can pass
through in sh_eval (csrc/embed.hip): the power recurrence costs two per step (a product and a fused multiply-add), 12 for a = 7; the
coefficient is rounded once; Horner in z^2 costs one per step plus one per use of the rounded z^2, at most 3 + 3, plus one for an odd
power's z; the final product one; a derivative's integer factor one more.  Longest: a = 7 value 12 + 1 + 1 = 14, a = 7 d/dx 10 + 1 + 1 + 1
= 13, (l, a) = (7, 1): 1 + 6 + 1 = 8.  K = 16 covers 15 first-order roundings and their second-order terms ((1 + 2^-24)^15 - 1 < 16 * 2^-24).
Half: that plus half an ulp of the result in half.
Frequency bound: tests/embedders_ref.py freq_value_tol with c = c_ref + 2 (c_ref is recorded in tests/golden/ref_embedders.npz);
backward and double backward: the restatement in fp64 on the kernel's own outputs, (2 n_freq + 2) * 2^-24 * sum |terms|.
Sizes: every B of SIZES up to 4099 runs for every degree / dtype and every (D, n_freq); B = 2^20 + 3 runs for SH degree 4 and 8 (both
dtypes) and for (D, n_freq) in (3, 6), (3, 10), (7, 16), (1, 0) only -- every listed value is hit at that size, not their product (the
fp64 restatement of a 231-column case at 2^20 rows is what costs, not the kernels)."""
import numpy as np
import pytest
import torch

import embedders_ref as R

pytestmark = pytest.mark.gpu

K = 16
TINY = 2.0 ** -126
SIZES = [0, 1, 63, 64, 65, 4099, 2 ** 20 + 3]


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _n(t):
    return t.detach().cpu().double().numpy()


def _points(B, seed):
    """in [-1, 1]^3: random off-sphere points, unit directions, the axes, the origin and the cube's corners"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (B, 3))
    if B >= 32:
        u = rng.standard_normal((B // 3, 3))
        p[:B // 3] = u / np.linalg.norm(u, axis=1, keepdims=True)
        p[-7:-1] = np.concatenate([np.eye(3), -np.eye(3)])
        p[-1] = 0
        p[-15:-7] = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)])
    return p.astype(np.float32)


def _half_ulp(ref, slack):
    return 0.5 * np.spacing((np.abs(ref) + slack).astype(np.float16)).astype(np.float64)


def _sh_fwd(x, degree, jac=False):
    from nr3d_lib_amd.bindings import _shencoder as S
    from nr3d_lib_amd import _hip as H
    B = x.shape[0]
    y = H.empty(B, degree * degree, dtype=x.dtype, device=x.device)
    j = H.empty(B, 3 * degree * degree, dtype=x.dtype, device=x.device) if jac else torch.empty(1, dtype=x.dtype, device=x.device)
    S.sh_encode_forward(x, y, B, 3, degree, jac, j)
    return (y, j.view(B, 3, degree * degree)) if jac else y


def _sh_bwd(g, x, degree, jac=None):
    from nr3d_lib_amd.bindings import _shencoder as S
    gx = torch.zeros_like(x)
    S.sh_encode_backward(g, x, x.shape[0], 3, degree, jac, gx)
    return gx


# ---- 5 / 6 / 7: SH values, derivatives, backward on both routes ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_values_jacobian_and_backward(dev, degree, dtype):
    half = dtype == torch.float16
    for B in SIZES:
        if B > 4099 and degree not in (4, 8):
            continue
        xh = _t(_points(B, 10 * degree + B % 7), dev, dtype)
        x64 = _n(xh)                                    # what the kernel sees (half inputs: the rounded values)
        y, jac = _sh_fwd(xh, degree, jac=True)
        assert y.shape == (B, degree * degree) and torch.equal(y, _sh_fwd(xh, degree))       # the Jacobian-free launch: same bytes
        Y, J = R.sh_all(x64, degree)
        M, MJ = R.sh_bound(x64, degree)
        by, bj = K * R.EPS * M + TINY, K * R.EPS * MJ + TINY
        if half:
            by, bj = by + _half_ulp(Y, by), bj + _half_ulp(J, bj)
        ey, ej = np.abs(_n(y) - Y), np.abs(_n(jac) - J)
        print(f"sh deg {degree} {dtype} B {B}: value err/bound {np.max(ey / by, initial=0):.3f}, jacobian {np.max(ej / bj, initial=0):.3f}")
        assert (ey <= by).all() and (ej <= bj).all()
        # backward: recompute vs stored Jacobian vs restatement.  dL/dx = sum_c g_c J_c: every J_c within its bound, C^2 + 1 roundings
        # of the fused sum on the absolute terms; the stored route rounds J to the storage type first (half: half an ulp of each J_c)
        rng = np.random.default_rng(B + degree)
        gh = _t(rng.standard_normal((B, degree * degree)).astype(np.float32), dev, dtype)
        g64 = _n(gh)
        want = np.einsum("bc,bdc->bd", g64, J)
        tol = np.einsum("bc,bdc->bd", np.abs(g64), bj) + (degree * degree + 1) * R.EPS * np.einsum("bc,bdc->bd", np.abs(g64), np.abs(J)) + TINY
        if half:
            tol = tol + _half_ulp(want, tol)
        rec, sto = _sh_bwd(gh, xh, degree), _sh_bwd(gh, xh, degree, jac.reshape(B, 3 * degree * degree))
        er, es = np.abs(_n(rec) - want), np.abs(_n(sto) - want)
        print(f"   backward err/bound: recompute {np.max(er / tol, initial=0):.3f}, stored {np.max(es / tol, initial=0):.3f}")
        assert (er <= tol).all() and (es <= tol).all()
        # the twin accumulates into grad_inputs
        from nr3d_lib_amd.bindings import _shencoder as S
        acc = torch.ones_like(xh)
        S.sh_encode_backward(gh, xh, B, 3, degree, None, acc)
        if not half:
            assert torch.equal(acc, 1 + rec)


def test_sh_bound_catches_a_wrong_coefficient(dev):
    """a change of one unit in the 4th digit of ANY coefficient must fail the bound on the seeded inputs (else K hides wrong tables): the
    value table against the value bound (and, being d/dx and d/dy's factor too, the Jacobian bound), the z-derivative table against the
    Jacobian bound"""
    x = _points(4099, 5)
    y, jac = _sh_fwd(_t(x, dev), 8, jac=True)
    y, jac = _n(y), _n(jac)
    M, MJ = R.sh_bound(x.astype(np.float64), 8)
    by, bj = K * R.EPS * M + TINY, K * R.EPS * MJ + TINY
    Y, J = R.sh_all(x, 8)
    assert (np.abs(y - Y) <= by).all() and (np.abs(jac - J) <= bj).all()
    for l in range(8):
        for a in range(l + 1):
            for t in range((l - a) // 2 + 1):
                bad_y, bad_j = R.sh_all(x, 8, perturb=(l, a, t, 1e-4))
                assert (np.abs(y - bad_y) > by).any(), ("value table", l, a, t)
                if a:                       # a = 0 columns have no d/dx, d/dy: their value table does not enter the Jacobian
                    assert (np.abs(jac - bad_j) > bj).any(), ("value table in the Jacobian", l, a, t)
            for t in range((l - a - 1) // 2 + 1 if a < l else 0):
                bad_y, bad_j = R.sh_all(x, 8, perturb=(l, a, t, 1e-4, 1))
                assert np.array_equal(bad_y, Y) and (np.abs(jac - bad_j) > bj).any(), ("z-derivative table", l, a, t)


@pytest.mark.parametrize("recompute", [True, False])
def test_sh_module_both_backward_routes(dev, recompute, monkeypatch):
    from nr3d_lib_amd.models.embedders import SHEncoder
    from nr3d_lib_amd.models.embedders.spherical_harmonics import sphere_harmonics as mod
    monkeypatch.setattr(mod, "RECOMPUTE_BACKWARD", recompute)
    p = _points(2 * 3 * 65, 3).reshape(2, 3, 65, 3)
    x = _t(p, dev).requires_grad_(True)
    enc = SHEncoder(3, 4)
    y = enc(x, size=2.0)
    assert y.shape == (2, 3, 65, 16)
    g = torch.randn_like(y)
    gx, = torch.autograd.grad(y, x, g)
    x64 = (x.detach() / 2.0).cpu().double().numpy().reshape(-1, 3)
    Y, J = R.sh_all(x64, 4)
    M, MJ = R.sh_bound(x64, 4)
    assert (np.abs(_n(y).reshape(-1, 16) - Y) <= K * R.EPS * M + TINY).all()
    g64 = _n(g).reshape(-1, 16)
    want = np.einsum("bc,bdc->bd", g64, J) / 2.0
    tol = (np.einsum("bc,bdc->bd", np.abs(g64), K * R.EPS * MJ) + 18 * R.EPS * np.einsum("bc,bdc->bd", np.abs(g64), np.abs(J))) / 2.0 + TINY
    assert (np.abs(_n(gx).reshape(-1, 3) - want) <= tol).all()
    # non-contiguous input (made contiguous), no gradient asked: no graph
    xt = _t(p.reshape(-1, 3), dev).t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(enc(xt), enc(xt.contiguous())) and not enc(xt).requires_grad
    # second order is refused, not silently dropped
    y2 = enc(x)
    g1, = torch.autograd.grad(y2, x, torch.ones_like(y2).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g1.sum().backward()
    # autocast: inputs are cast to float32
    with torch.autocast("cuda", dtype=torch.float16):
        assert enc(x.detach().half()).dtype == torch.float32


# ---- 5 / 6: frequency values, backward, double backward ------------------------------------------------------------------------------
def _freq_fwd(x, n):
    from nr3d_lib_amd.bindings import _freqencoder as F
    from nr3d_lib_amd import _hip as H
    B, D = x.shape
    y = H.empty(B, R.freq_cols(D, n), dtype=torch.float32, device=x.device)
    F.freq_encode_forward(x, B, D, n, y.shape[1], y)
    return y


@pytest.fixture(scope="module")
def c_ref():
    import os
    return float(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_embedders.npz"))["c_ref"])


@pytest.mark.parametrize("n", [0, 1, 6, 10, 16])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 7])
def test_freq_values_backward_double_backward(dev, c_ref, D, n):
    from nr3d_lib_amd.bindings import _freqencoder as F
    from nr3d_lib_amd import _hip as H
    C = R.freq_cols(D, n)
    for B in SIZES:
        if B > 4099 and (D, n) not in ((3, 6), (3, 10), (7, 16), (1, 0)):
            continue
        rng = np.random.default_rng(100 * D + n + B % 5)
        x = rng.uniform(-1, 1, (B, D)).astype(np.float32)
        if B > 8:
            x[:3] = [[0.0], [1.0], [-1.0]]
        xt = _t(x, dev)
        y = _freq_fwd(xt, n)
        err, tol = np.abs(_n(y) - R.freq_forward(x, n)), R.freq_value_tol(x, n, c_ref + 2)
        resid = (err - R.freq_arg_term(x, n))[:, D:]
        print(f"freq D {D} n {n} B {B}: c measured {np.max(resid, initial=0) / R.EPS:.3f} (allowed {c_ref + 2:.3f})")
        assert torch.equal(y[:, :D], xt) and (err <= tol).all()
        g = rng.standard_normal((B, C)).astype(np.float32)
        v = rng.standard_normal((B, D)).astype(np.float32)
        gt, vt = _t(g, dev), _t(v, dev)
        gx = H.empty(B, D, dtype=torch.float32, device=dev)
        F.freq_encode_backward(gt, y, B, D, n, C, gx)
        y64 = _n(y)
        want, tolb = R.freq_backward(g, y64, D, n), (2 * n + 2) * R.EPS * R.freq_backward(g, y64, D, n, absolute=True)
        assert (np.abs(_n(gx) - want) <= tolb).all()
        dg, dx = H.empty(B, C, dtype=torch.float32, device=dev), H.empty(B, D, dtype=torch.float32, device=dev)
        F.freq_encode_backward_backward(vt, gt, y, B, D, n, C, dg, dx)
        wg, wx = R.freq_backward_backward(v, g, y64, D, n)
        ag, ax = R.freq_backward_backward(v, g, y64, D, n, absolute=True)
        assert (np.abs(_n(dg) - wg) <= (2 * n + 2) * R.EPS * ag).all() and (np.abs(_n(dx) - wx) <= (2 * n + 2) * R.EPS * ax).all()
        # each output alone: the same bytes
        dg1, dx1 = H.empty(B, C, dtype=torch.float32, device=dev), H.empty(B, D, dtype=torch.float32, device=dev)
        F.freq_encode_backward_backward(vt, gt, y, B, D, n, C, dg1, None)
        F.freq_encode_backward_backward(vt, gt, y, B, D, n, C, None, dx1)
        assert torch.equal(dg1, dg) and torch.equal(dx1, dx)


def test_freq_module_shapes_dtypes_and_autocast(dev):
    from nr3d_lib_amd.models.embedders import FreqEncoder, get_embedder
    enc, C = get_embedder({"type": "sinusoidal", "n_frequencies": 6}, 3)
    x = _t(np.random.default_rng(0).uniform(-1, 1, (2, 5, 7, 3)).astype(np.float32), dev)
    y = enc(x)
    assert y.shape == (2, 5, 7, 39) and C == 39 and torch.equal(y.reshape(-1, 39), _freq_fwd(x.reshape(-1, 3), 6))
    xt = x.reshape(-1, 3).t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(enc(xt), y.reshape(-1, 39))
    with pytest.raises(RuntimeError, match="Float"):
        enc(x.double())
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(enc(x.half()), enc(x.half().float()))
    assert FreqEncoder(3, 0)(x).equal(x)


# ---- 8: output into a column slice of a wider buffer -------------------------------------------------------------------------------------
def test_output_into_a_column_slice(dev):
    from nr3d_lib_amd.bindings import _shencoder as S, _freqencoder as F
    from nr3d_lib_amd import _hip as H
    assert H.POISON
    B = 4099
    x = _t(_points(B, 8), dev)
    for dtype, degree, off, width in ((torch.float32, 4, 4, 24), (torch.float32, 3, 5, 19), (torch.float16, 4, 8, 32), (torch.float16, 5, 3, 31)):
        xd = x.to(dtype)
        wide = H.empty(B, width, dtype=dtype, device=dev)
        before = wide.clone()
        S.sh_encode_into(xd, wide[:, off:off + degree * degree], degree)
        assert torch.equal(wide[:, off:off + degree * degree], _sh_fwd(xd, degree))
        keep = torch.ones(width, dtype=torch.bool, device=dev)
        keep[off:off + degree * degree] = False
        assert torch.equal(wide[:, keep].view(torch.int16 if dtype == torch.float16 else torch.int32),
                           before[:, keep].view(torch.int16 if dtype == torch.float16 else torch.int32))
    for off, width in ((4, 48), (1, 41)):
        wide = H.empty(B, width, dtype=torch.float32, device=dev)
        before = wide.clone()
        F.freq_encode_into(x, wide[:, off:off + 39], 6)
        assert torch.equal(wide[:, off:off + 39], _freq_fwd(x, 6))
        keep = torch.ones(width, dtype=torch.bool, device=dev)
        keep[off:off + 39] = False
        assert torch.equal(wide[:, keep].view(torch.int32), before[:, keep].view(torch.int32))


# ---- 9: frequency second order end to end ---------------------------------------------------------------------------------------------------
def test_freq_second_order_matches_the_legacy_embedder_in_fp64(dev, c_ref):
    from nr3d_lib_amd.models.embedders import FreqEncoder, get_sinusoidal_embedder
    rng = np.random.default_rng(9)
    B, n = 4099, 6
    xn, gn = rng.uniform(-1, 1, (B, 3)).astype(np.float32), rng.standard_normal((B, 39)).astype(np.float32)

    def program(embed, dtype, device):
        x = torch.from_numpy(xn).to(device=device, dtype=dtype).requires_grad_(True)
        g = torch.from_numpy(gn).to(device=device, dtype=dtype).requires_grad_(True)
        h = embed(x)
        nab, = torch.autograd.grad(h, x, g, create_graph=True)
        ((nab.norm(dim=-1) - 1) ** 2).mean().backward()
        return nab, x, g

    nab, x, g = program(FreqEncoder(3, n), torch.float32, dev)
    nab64, x64, g64 = program(get_sinusoidal_embedder(n, 3)[0].double(), torch.float64, "cpu")
    c = c_ref + 2
    y_exact = R.freq_forward(xn, n)
    assert (np.abs(_n(nab) - nab64.detach().numpy()) <= R.freq_grad_tol(xn, gn, n, c, y_exact)).all()
    tol_dg, tol_dx = R.eikonal_tols(xn, gn, n, c)
    eg, ex = np.abs(_n(g.grad) - g64.grad.numpy()), np.abs(_n(x.grad) - x64.grad.numpy())
    print(f"eikonal: g.grad err/bound {np.max(eg / tol_dg):.3f}, x.grad err/bound {np.max(ex / tol_dx):.3f}")
    assert (eg <= tol_dg).all() and (ex <= tol_dx).all()
    P = R.eikonal_program(xn, gn, n)                       # the torch program in fp64 and the restatement are the same function
    assert np.allclose(P["dx"], x64.grad.numpy(), rtol=1e-9, atol=1e-15) and np.allclose(P["dg"], g64.grad.numpy(), rtol=1e-9, atol=1e-15)
    # third order raises
    x3 = torch.from_numpy(xn).to(dev).requires_grad_(True)
    g3 = torch.from_numpy(gn).to(dev).requires_grad_(True)
    n3, = torch.autograd.grad(FreqEncoder(3, n)(x3), x3, g3, create_graph=True)
    s3, = torch.autograd.grad((n3 ** 2).sum(), x3, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        s3.sum().backward()


@pytest.mark.parametrize("case", ["column_slice", "transposed", "autocast_slice", "autocast_half"])
def test_freq_second_order_reaches_the_leaf_through_views_and_casts(dev, c_ref, case):
    """the eikonal program on an x that is NOT the contiguous float32 tensor the kernels take: a column slice of a wider leaf, a
    transposed view, the same inside an autocast region, and a half tensor cast by the region.  leaf.grad must carry the double
    backward's dL/dx (a copy made where autograd does not see it would drop it without an error)."""
    from nr3d_lib_amd.models.embedders import FreqEncoder, get_sinusoidal_embedder
    rng = np.random.default_rng(19)
    B, n = 1031, 6
    wide = rng.uniform(-1, 1, (B, 5)).astype(np.float32)
    gn = rng.standard_normal((B, 39)).astype(np.float32)
    half = case == "autocast_half"
    if half:
        wide = wide.astype(np.float16).astype(np.float32)           # the values the kernel will see
    xn = wide[:, 1:4]

    def view(leaf):
        return leaf.t()[:, 1:4] if case == "transposed" else leaf[:, 1:4]

    leaf = torch.from_numpy(np.ascontiguousarray(wide.T) if case == "transposed" else wide).to(dev)
    leaf = (leaf.half() if half else leaf).requires_grad_(True)
    g = torch.from_numpy(gn).to(dev).requires_grad_(True)
    x = view(leaf)
    assert not x.is_contiguous()
    with torch.autocast("cuda", dtype=torch.float16, enabled=case.startswith("autocast")):
        h = FreqEncoder(3, n)(x)
        assert h.dtype == torch.float32
        nab, = torch.autograd.grad(h, x, g, create_graph=True)
        ((nab.float().norm(dim=-1) - 1) ** 2).mean().backward()
    assert leaf.grad is not None and g.grad is not None
    lg = view(leaf.grad)
    other = torch.ones(5, dtype=torch.bool)
    other[1:4] = False
    assert not (leaf.grad.t() if case == "transposed" else leaf.grad)[:, other].any()      # the columns outside the view get zeros
    if half:
        # nab reaches the loss as a half tensor (the gradient of a half view), so the fp64 program differs by half roundings that this
        # test does not bound: the point here is that the gradient arrives at all, finite and not zero
        assert torch.isfinite(lg).all() and lg.abs().sum() > 0 and torch.isfinite(g.grad).all()
        return
    x64 = torch.from_numpy(xn).double().requires_grad_(True)
    g64 = torch.from_numpy(gn).double().requires_grad_(True)
    n64, = torch.autograd.grad(get_sinusoidal_embedder(n, 3)[0].double()(x64), x64, g64, create_graph=True)
    ((n64.norm(dim=-1) - 1) ** 2).mean().backward()
    tol_dg, tol_dx = R.eikonal_tols(xn, gn, n, c_ref + 2)
    assert (np.abs(_n(nab) - n64.detach().numpy()) <= R.freq_grad_tol(xn, gn, n, c_ref + 2, R.freq_forward(xn, n))).all()
    assert (np.abs(_n(lg) - x64.grad.numpy()) <= tol_dx).all() and (np.abs(_n(g.grad) - g64.grad.numpy()) <= tol_dg).all()


def test_backward_reads_from_column_slices(dev):
    """grad_stride of nr3d_sh_encode_bwd, y_stride of nr3d_freq_encode_bwd / _bwd_bwd: inputs that are column slices of wider buffers give
    the bytes of the contiguous call (16-byte and element-wise read paths)"""
    from nr3d_lib_amd.bindings import _freqencoder as F
    from nr3d_lib_amd import _hip as H
    L, B = H.lib(), 4099
    x = _t(_points(B, 21), dev)
    st = H.stream_of(x)
    for dtype, degree, off, width in ((torch.float32, 4, 4, 24), (torch.float32, 3, 5, 19), (torch.float16, 4, 8, 32), (torch.float16, 5, 3, 31)):
        xd, W = x.to(dtype), degree * degree
        wide = torch.randn(B, width, device=dev).to(dtype)
        g = wide[:, off:off + W]
        want = _sh_bwd(g.contiguous(), xd, degree)
        y, jac = _sh_fwd(xd, degree, jac=True)
        for j in (None, jac):
            gx = H.empty(B, 3, dtype=dtype, device=dev)
            H.check(L.nr3d_sh_encode_bwd(B, 3, degree, H.DTYPE_CODE[dtype], g.data_ptr(), width, xd.data_ptr(), H.ptr(j), gx.data_ptr(), 0, st))
            assert torch.equal(gx, want if j is None else _sh_bwd(g.contiguous(), xd, degree, jac.reshape(B, 3 * W)))
    n, C = 6, 39
    y = _freq_fwd(x, n)
    g, v = torch.randn(B, C, device=dev), torch.randn(B, 3, device=dev)
    gx, dg, dx = H.empty(B, 3, dtype=torch.float32, device=dev), H.empty(B, C, dtype=torch.float32, device=dev), H.empty(B, 3, dtype=torch.float32, device=dev)
    F.freq_encode_backward(g, y, B, 3, n, C, gx)
    F.freq_encode_backward_backward(v, g, y, B, 3, n, C, dg, dx)
    for off, width in ((4, 48), (1, 41)):
        wide = H.empty(B, width, dtype=torch.float32, device=dev)
        ys = wide[:, off:off + C]
        F.freq_encode_into(x, ys, n)
        gx2, dg2, dx2 = torch.empty_like(gx), torch.empty_like(dg), torch.empty_like(dx)
        H.check(L.nr3d_freq_encode_bwd(B, 3, n, C, g.data_ptr(), ys.data_ptr(), width, gx2.data_ptr(), st))
        H.check(L.nr3d_freq_encode_bwd_bwd(B, 3, n, C, v.data_ptr(), g.data_ptr(), ys.data_ptr(), width, dg2.data_ptr(), dx2.data_ptr(), st))
        assert torch.equal(gx2, gx) and torch.equal(dg2, dg) and torch.equal(dx2, dx)


# ---- 10: non-finite rows ------------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_stay_in_their_rows(dev):
    from nr3d_lib_amd.bindings import _freqencoder as F
    B = 257
    p = _points(B, 11)
    bad_rows = {7: np.nan, 64: np.inf, 200: -np.inf}
    q = p.copy()
    for r, val in bad_rows.items():
        q[r, r % 3] = val
    good = np.array([r not in bad_rows for r in range(B)])
    x, xb = _t(p, dev), _t(q, dev)
    g = torch.randn(B, 64, device=dev)
    y, yb = _sh_fwd(x, 8), _sh_fwd(xb, 8)
    gx, gxb = _sh_bwd(g, x, 8), _sh_bwd(g, xb, 8)
    assert torch.equal(y[good], yb[good]) and torch.equal(gx[good], gxb[good])
    for r in bad_rows:
        assert yb[r, 0] == y[r, 0] and not torch.isfinite(yb[r, 1:]).all() and not torch.isfinite(gxb[r]).all()
    g = torch.randn(B, 39, device=dev)
    y, yb = _freq_fwd(x, 6), _freq_fwd(xb, 6)
    gx, gxb = torch.empty_like(x), torch.empty_like(x)
    F.freq_encode_backward(g, y, B, 3, 6, 39, gx)
    F.freq_encode_backward(g, yb, B, 3, 6, 39, gxb)
    assert torch.equal(y[good], yb[good]) and torch.equal(gx[good], gxb[good])
    for r in bad_rows:
        assert not torch.isfinite(yb[r]).all() and not torch.isfinite(gxb[r]).all()
        d = r % 3
        ok = [c for c in range(39) if c % 3 != d]
        assert torch.equal(yb[r, ok], y[r, ok])           # the row's other input dimensions are untouched as well
    v = torch.randn(B, 3, device=dev)
    dg, dx, dgb, dxb = torch.empty_like(g), torch.empty_like(x), torch.empty_like(g), torch.empty_like(x)
    F.freq_encode_backward_backward(v, g, y, B, 3, 6, 39, dg, dx)
    F.freq_encode_backward_backward(v, g, yb, B, 3, 6, 39, dgb, dxb)
    assert torch.equal(dg[good], dgb[good]) and torch.equal(dx[good], dxb[good])
    for r in bad_rows:
        assert not torch.isfinite(dgb[r]).all() and not torch.isfinite(dxb[r]).all()


# ---- 11: determinism -----------------------------------------------------------------------------------------------------------------------
def test_every_kernel_is_deterministic(dev):
    from nr3d_lib_amd.bindings import _freqencoder as F
    B = 2 ** 18 + 5
    x = _t(_points(B, 12), dev)

    def run():
        out = []
        for dtype in (torch.float32, torch.float16):
            xd = x.to(dtype)
            g = torch.ones(B, 16, device=dev, dtype=dtype) * 0.37
            y, j = _sh_fwd(xd, 4, jac=True)
            out += [y, j, _sh_bwd(g, xd, 4), _sh_bwd(g, xd, 4, j.reshape(B, 48))]
        y = _freq_fwd(x, 10)
        g = torch.sin(torch.arange(B * 63, device=dev, dtype=torch.float32)).view(B, 63)
        gx, dg, dx = torch.empty_like(x), torch.empty_like(g), torch.empty_like(x)
        F.freq_encode_backward(g, y, B, 3, 10, 63, gx)
        F.freq_encode_backward_backward(gx, g, y, B, 3, 10, 63, dg, dx)
        return out + [y, gx, dg, dx]

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)


# ---- 12: model level ------------------------------------------------------------------------------------------------------------------------
def test_mlpnet_with_sh_embedding_on_the_fused_decoder(dev):
    from nr3d_lib_amd.models.blocks.mlp import MLPNet
    torch.manual_seed(0)
    net = MLPNet(3, 3, embed_cfg={"type": "spherical", "degree": 4}, D=1, W=32).to(dev)
    p = _points(4099, 13)
    x = _t(p, dev).requires_grad_(True)
    h = net.embedder(x)
    assert net._fused_ok(h, False, None) is not None          # the block takes the fused decoder kernel on the embedder's output
    y = net(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    # the SH restatement followed by the same MLP, layer by layer in fp64
    Y, J = R.sh_all(p.astype(np.float64), 4)
    e = torch.from_numpy(Y).requires_grad_(True)
    ws = [(l.weight.detach().double().cpu().requires_grad_(True), l.bias.detach().double().cpu().requires_grad_(True)) for l in net.layers]
    h64 = torch.relu(torch.nn.functional.linear(e, *ws[0]))
    y64 = torch.nn.functional.linear(h64, *ws[1])
    y64.backward(gy.double().cpu())
    gx64 = torch.einsum("bc,bdc->bd", e.grad, torch.from_numpy(J))
    torch.testing.assert_close(y.detach().double().cpu(), y64.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(x.grad.double().cpu(), gx64, rtol=1e-4, atol=1e-5)
    for l, (w, b) in zip(net.layers, ws):
        torch.testing.assert_close(l.weight.grad.double().cpu(), w.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(l.bias.grad.double().cpu(), b.grad, rtol=1e-4, atol=1e-5)
