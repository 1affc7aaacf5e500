"""GPU: the fused NeuS opacity (csrc/neus_alpha.hip through bindings._neus_alpha and graphics/neus/neus_utils.py under
FUSED_SDF_TO_ALPHA) against the reference's op chain restated in torch (tests/neus_alpha_ref.py).

Yardstick, in the form of tests/test_mlp_second_order_gpu.py: for alpha, dL/dsdf and dL/dappends the error against the float64
evaluation, relative to the tensor's maximum, stays within max(1e-5, 4 x the error of torch's fp32 chain on the same inputs and
device).  For the scalar dL/dinv_s, a sum that cancels by orders of magnitude: |dL/dinv_s - float64| <= 4 x max(|torch fp32 chain -
float64|, eps32 T), T = the float64 sum of the absolute un-cancelled contributions (one rounding per contribution).  Every check
prints its ratio ("YARDSTICK ..."); profiles/neus_alpha.json keeps one run of them: 1103 checks, the largest ratios 1.84 (alpha), 2.78
(dL/dsdf), 2.0 (dL/dinv_s); dL/dappends reaches 144 at an error of 1.4e-07, below the 1e-5 floor.
The float64 evaluation writes its sigmoid so that autograd's derivative is E / (1 + E)^2 (neus_alpha_ref._sigmoid64): with torch.sigmoid
in float64 the derivative is exactly 0 from z = 36.8 on, and on rows 7x2 "noisy" at inv_s 256, where all of dL/dsdf is below 2e-25 and
such entries carry it, that reference put the kernel -- and the true value -- at a relative error of 4.32.

Input condition, asserted: no interval of the inputs has 0 < |z_i - z_next| < 1e-4 in float64 (so near a tie that float32 and float64
could take different sides of the clamp), so no element is left out of any comparison; exact ties ("flat") are wanted.
The tests set FUSED_SDF_TO_ALPHA themselves, so they cover the fused route whatever its default is."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

import neus_alpha_ref as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
FUSED_NODE = "_SdfToAlphaBackward"
MODES = ("none", "one", "sdf")                 # the interval after a pack's last sample: none, against cdf 1, against an appended SDF


@contextlib.contextmanager
def _switch(on):
    from nr3d_lib_amd.graphics.neus import neus_utils as nu
    saved = nu.FUSED_SDF_TO_ALPHA
    nu.FUSED_SDF_TO_ALPHA = on
    try:
        yield nu
    finally:
        nu.FUSED_SDF_TO_ALPHA = saved


def _check(name, got, ref64, ref32):
    scale = float(ref64.abs().max()) or 1.0
    err = float((got.double() - ref64.double()).abs().max()) / scale
    err32 = float((ref32.double() - ref64.double()).abs().max()) / scale
    print(f"YARDSTICK {name}: rel err {err:.3e} torch fp32 {err32:.3e} ratio {err / err32 if err32 else float('inf'):.2f}")
    assert torch.isfinite(got).all(), f"{name}: not finite"
    assert err <= max(1e-5, 4 * err32), f"{name}: rel err {err:.2e} (torch fp32 chain: {err32:.2e})"


def _check_scalar(name, got, r64, r32):
    want, T = float(r64["g_inv_s"]), r64["T"]
    err, err32 = abs(float(got) - want), abs(float(r32["g_inv_s"]) - want)
    print(f"YARDSTICK {name}: err {err:.3e} torch fp32 {err32:.3e} eps32 T {EPS32 * T:.3e} "
          f"ratio {err / max(err32, EPS32 * T) if T else float('inf'):.2f}")
    assert np.isfinite(float(got)), f"{name}: not finite"
    assert err <= 4 * max(err32, EPS32 * T), f"{name}: err {err:.2e} (torch fp32 chain: {err32:.2e}, eps32 T: {EPS32 * T:.2e})"


@functools.lru_cache(maxsize=None)
def _pack_case(kind, seed, layout):
    """the inputs on the GPU, computed once: (sdf, pack_infos -- marked ordered unless shuffled --, appends, g)"""
    from nr3d_lib_amd import _hip
    dev = torch.device("cuda:0")
    sdf, pi, app, g = (t.to(dev) for t in ref.packs(kind, seed, layout=layout))
    if layout != "shuffled":
        _hip.mark_ordered(pi)
    for inv_s in ref.INV_S:
        assert ref.near_ties(sdf, inv_s, pi, app) == 0, "input condition"
    return sdf, pi, app, g


@functools.lru_cache(maxsize=None)
def _pack_refs(kind, seed, layout, inv_s, mode):
    sdf, pi, app, g = _pack_case(kind, seed, layout)
    kw = dict(pack_infos=pi, append_cdf_1=mode == "one", appends=app if mode == "sdf" else None)
    return ref.chain(sdf, inv_s, g, dtype=torch.float64, **kw), ref.chain(sdf, inv_s, g, dtype=torch.float32, **kw)


@functools.lru_cache(maxsize=None)
def _row_case(kind, seed, n, R=7):
    dev = torch.device("cuda:0")
    sdf, g = (t.to(dev) for t in ref.rows(kind, seed, R, n))
    for inv_s in ref.INV_S:
        assert ref.near_ties(sdf, inv_s) == 0, "input condition"
    return sdf, g


@functools.lru_cache(maxsize=None)
def _row_refs(kind, seed, n, inv_s, append):
    sdf, g = _row_case(kind, seed, n)
    return (ref.chain(sdf, inv_s, g, append_cdf_1=append, dtype=torch.float64),
            ref.chain(sdf, inv_s, g, append_cdf_1=append, dtype=torch.float32))


def _run(sdf, inv_s, g, pi=None, mode="none", app=None, fused=True, inv_s_shape=()):
    """forward + backward through neus_utils with a learnable inv_s on the GPU -> (alpha, dL/dsdf, dL/dappends | None, dL/dinv_s, node)"""
    x = sdf.clone().requires_grad_(True)
    s = torch.full(inv_s_shape, inv_s, device=sdf.device).requires_grad_(True)
    a = app.clone().requires_grad_(True) if mode == "sdf" else None
    with _switch(fused) as nu:
        if pi is None:
            alpha = nu.neus_ray_sdf_to_alpha(x, s, append_cdf_1=mode == "one")
        else:
            alpha = nu.neus_packed_sdf_to_alpha(x, s, pi, append_cdf_1=mode == "one", pack_sdf_appends=a)
        alpha.backward(g if alpha.shape == g.shape else g[..., :-1])
    return alpha.detach(), x.grad, None if a is None else a.grad, s.grad, type(alpha.grad_fn).__name__


def _outside(pi, S, dev):
    inside = torch.zeros(S, dtype=torch.bool, device=dev)
    for b, n in pi.tolist():
        inside[b:b + n] = True
    return ~inside


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("layout", ["contiguous", "gaps", "shuffled"])
def test_packed_matches_the_chain(dev, layout, kind, mode):
    for seed in (0, 1):
        sdf, pi, app, g = _pack_case(kind, seed, layout)
        out = _outside(pi, sdf.numel(), dev)
        last = (pi[:, 0] + pi[:, 1] - 1)[pi[:, 1] > 0]
        for inv_s in ref.INV_S:
            r64, r32 = _pack_refs(kind, seed, layout, inv_s, mode)
            alpha, g_sdf, g_app, g_inv_s, node = _run(sdf, inv_s, g, pi, mode, app)
            assert node == FUSED_NODE
            tag = f"packed {layout} {kind} seed {seed} inv_s {inv_s:g} append {mode}"
            _check(f"{tag} alpha", alpha, r64["alpha"], r32["alpha"])
            _check(f"{tag} dL/dsdf", g_sdf, r64["g_sdf"], r32["g_sdf"])
            if mode == "sdf":
                _check(f"{tag} dL/dappends", g_app, r64["g_appends"], r32["g_appends"])
            _check_scalar(f"{tag} dL/dinv_s", g_inv_s, r64, r32)
            # rows outside every pack: exactly 0 (the poison fill of the test run would show a miss), ordered and unordered
            assert out.sum() > 0 or layout == "contiguous"
            assert bool((alpha[out] == 0).all()) and bool((g_sdf[out] == 0).all())
            if mode == "none":
                assert bool((alpha[last] == 0).all())
            if kind == "flat":                      # the constant intervals: alpha 0, and the gradient passes at equality
                tie = ref.chain(sdf, inv_s, pack_infos=pi, append_cdf_1=False)["alpha"] == 0
                tie &= ~out
                tie[last] = False
                assert tie.sum() > sdf.numel() // 2 and bool((alpha[tie] == 0).all())
                zero = tie & (g_sdf == 0)                    # g is randn, never 0: every tie sample has a gradient
                assert not bool(zero.any()), f"{tag}: dL/dsdf is 0 on the constant intervals at {zero.nonzero().flatten().tolist()}"


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("n", [2, 3, 64, 65, 130])
def test_rows_match_the_chain(dev, n, append):
    for kind in ref.KINDS:
        for seed in (0, 1):
            sdf, g = _row_case(kind, seed, n)
            for inv_s in ref.INV_S:
                r64, r32 = _row_refs(kind, seed, n, inv_s, append)
                alpha, g_sdf, _, g_inv_s, node = _run(sdf, inv_s, g, mode="one" if append else "none")
                assert node == FUSED_NODE and alpha.shape == (7, n if append else n - 1)
                tag = f"rows 7x{n} {kind} seed {seed} inv_s {inv_s:g} append {int(append)}"
                _check(f"{tag} alpha", alpha, r64["alpha"], r32["alpha"])
                _check(f"{tag} dL/dsdf", g_sdf, r64["g_sdf"], r32["g_sdf"])
                _check_scalar(f"{tag} dL/dinv_s", g_inv_s, r64, r32)


def test_rows_of_one_sample(dev, monkeypatch):
    """n = 1 without append: an empty result, zero gradients, and no launch"""
    from nr3d_lib_amd import _hip
    calls, real_check = [], _hip.check
    sdf = torch.randn(7, 1, device=dev)
    with _switch(True) as nu:
        x = sdf.clone().requires_grad_(True)
        s = torch.tensor(64.0, device=dev, requires_grad=True)
        monkeypatch.setattr(nu._backend.H, "check", lambda rc: calls.append(rc) or real_check(rc))
        alpha = nu.neus_ray_sdf_to_alpha(x, s)
        assert alpha.shape == (7, 0) and type(alpha.grad_fn).__name__ == FUSED_NODE
        alpha.sum().backward()
        assert calls == [] and bool((x.grad == 0).all()) and float(s.grad) == 0.0
        one = nu.neus_ray_sdf_to_alpha(sdf, 64.0, append_cdf_1=True)
        assert one.shape == (7, 1) and len(calls) == 1
        torch.testing.assert_close(one, nu.neus_ray_sdf_to_alpha(sdf, 64.0, append_cdf_1=True, fused=False), rtol=1e-5, atol=1e-6)


def test_route(dev, monkeypatch):
    """the fused Function where the route applies and the chain (equal results) where it does not; one binding call each way per use"""
    from nr3d_lib_amd.bindings import _neus_alpha as B
    count = dict(fwd=0, bwd=0)
    real_f, real_b = B.sdf_to_alpha_forward, B.sdf_to_alpha_backward
    monkeypatch.setattr(B, "sdf_to_alpha_forward", lambda *a, **k: count.__setitem__("fwd", count["fwd"] + 1) or real_f(*a, **k))
    monkeypatch.setattr(B, "sdf_to_alpha_backward", lambda *a, **k: count.__setitem__("bwd", count["bwd"] + 1) or real_b(*a, **k))
    sdf, pi, app, g = _pack_case("noisy", 0, "gaps")
    rows, g_rows = _row_case("noisy", 0, 65)
    with _switch(True) as nu:
        for use in (lambda x, s: nu.neus_packed_sdf_to_alpha(x, s, pi), lambda x, s: nu.neus_packed_sdf_to_alpha(x, s, pi, True),
                    lambda x, s: nu.neus_packed_sdf_to_alpha(x, s, pi, pack_sdf_appends=app),
                    lambda x, s: nu.neus_packed_sdf_to_vw(x, s, pi)):
            count.update(fwd=0, bwd=0)
            x, s = sdf.clone().requires_grad_(True), torch.tensor(256.0, device=dev, requires_grad=True)
            out = use(x, s)
            out.backward(g)
            assert count == dict(fwd=1, bwd=1)
        count.update(fwd=0, bwd=0)
        x = rows.clone().requires_grad_(True)
        alpha = nu.neus_ray_sdf_to_alpha(x, 256.0)                          # a Python number: no dL/dinv_s, one launch each way
        assert type(alpha.grad_fn).__name__ == FUSED_NODE
        alpha.backward(g_rows[:, :-1])
        assert count == dict(fwd=1, bwd=1)
        with torch.no_grad():
            assert torch.equal(nu.neus_ray_sdf_to_alpha(rows, 256.0), alpha) and count["fwd"] == 2      # no_grad: the same kernel, the same bits
        assert torch.equal(nu.neus_ray_sdf_to_alpha(rows, 256.0), alpha) and count["fwd"] == 3          # nothing requires grad
        # the chain: fused=False, a half sdf, a per-sample inv_s, a double sdf
        count.update(fwd=0, bwd=0)
        per_sample = torch.full_like(rows, 256.0)
        for x, s, kw in ((rows, 256.0, dict(fused=False)), (rows.half(), 256.0, {}), (rows, per_sample, {}), (rows.double(), 256.0, {})):
            x = x.clone().requires_grad_(True)
            a_on = nu.neus_ray_sdf_to_alpha(x, s, **kw)
            assert type(a_on.grad_fn).__name__ != FUSED_NODE
            with _switch(False):
                assert torch.equal(a_on, nu.neus_ray_sdf_to_alpha(x, s))
        x = sdf.clone().requires_grad_(True)
        a_on = nu.neus_packed_sdf_to_alpha(x, 256.0, pi, fused=False)
        assert type(a_on.grad_fn).__name__ != FUSED_NODE
        with _switch(False):
            assert torch.equal(a_on, nu.neus_packed_sdf_to_alpha(x, 256.0, pi))
        assert count == dict(fwd=0, bwd=0)
    with _switch(False) as nu:
        x = rows.clone().requires_grad_(True)
        assert type(nu.neus_ray_sdf_to_alpha(x, 256.0).grad_fn).__name__ != FUSED_NODE
        assert type(nu.neus_ray_sdf_to_alpha(x, 256.0, fused=True).grad_fn).__name__ == FUSED_NODE


@pytest.mark.parametrize("append", [False, True])
def test_same_bits_in_both_layouts(dev, append):
    """rows [R, n] and the same data as R ordered packs of n: the same alpha and dL/dsdf; grad mode and no_grad: the same alpha"""
    from nr3d_lib_amd import _hip
    for n in (3, 65, 130):
        sdf, g = _row_case("noisy", 1, n)
        pi = _hip.mark_ordered(ref.row_pack_infos(7, n, dev))
        mode = "one" if append else "none"
        a_rows, gs_rows, _, gi_rows, _ = _run(sdf, 256.0, g, mode=mode)
        g_flat = g.clone()
        if not append:
            g_flat[:, -1] = 123.0                                           # the last sample of a pack closes no interval: g is not read
        a_pack, gs_pack, _, gi_pack, _ = _run(sdf.flatten(), 256.0, g_flat.flatten(), pi, mode)
        a_pack = a_pack.reshape(7, n)
        if not append:
            assert bool((a_pack[:, -1] == 0).all())
            a_pack = a_pack[:, :-1]
        assert torch.equal(a_rows, a_pack) and torch.equal(gs_rows.flatten(), gs_pack)
        with torch.no_grad(), _switch(True) as nu:
            assert torch.equal(nu.neus_ray_sdf_to_alpha(sdf, torch.tensor(256.0, device=dev), append_cdf_1=append), a_rows)


def test_same_bits_run_to_run(dev):
    sdf, pi, app, g = _pack_case("noisy", 0, "gaps")
    rows, g_rows = _row_case("noisy", 0, 130)
    for args in ((sdf, 256.0, g, pi, "sdf", app), (sdf, 2048.0, g, _pack_case("noisy", 0, "shuffled")[1], "none", app),
                 (rows, 256.0, g_rows, None, "one", None)):
        first = _run(*args)
        again = _run(*args)
        for a, b in zip(first[:4], again[:4]):
            assert (a is None and b is None) or torch.equal(a, b)


def test_last_sample_without_append(dev):
    """no append: g at the last sample of every pack reaches no gradient"""
    for layout in ("gaps", "shuffled"):
        sdf, pi, app, g = _pack_case("cross", 0, layout)
        last = (pi[:, 0] + pi[:, 1] - 1)[pi[:, 1] > 0]
        g2 = g.clone()
        g2[last] = 1e6
        a = _run(sdf, 256.0, g, pi, "none")
        b = _run(sdf, 256.0, g2, pi, "none")
        assert bool((a[0][last] == 0).all()) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])


def test_inv_s_forms(dev):
    """a GPU parameter gets a .grad of its own shape; a float, a CPU 0-dim tensor and GPU tensors of the same value: the same alpha bits"""
    sdf, pi, app, g = _pack_case("noisy", 1, "contiguous")
    want = None
    for shape in ((), (1,), (1, 1)):
        alpha, _, _, g_inv_s, node = _run(sdf, 256.0, g, pi, "one", inv_s_shape=shape)
        assert node == FUSED_NODE and g_inv_s.shape == shape and g_inv_s.is_cuda
        want = alpha if want is None else want
        assert torch.equal(alpha, want)
    with _switch(True) as nu:
        for inv_s in (256.0, 256, torch.tensor(256.0), torch.tensor(256.0, dtype=torch.float64), torch.tensor(256.0, device=dev)):
            x = sdf.clone().requires_grad_(True)
            alpha = nu.neus_packed_sdf_to_alpha(x, inv_s, pi, append_cdf_1=True)
            assert type(alpha.grad_fn).__name__ == FUSED_NODE and torch.equal(alpha.detach(), want)


@pytest.mark.parametrize("layout,mode", [("packed", "none"), ("packed", "one"), ("packed", "sdf"), ("rows", "none"), ("rows", "one")])
def test_create_graph(dev, layout, mode):
    """double backward: the first backward under create_graph returns differentiable torch ops, the second one runs and gives the
    second-order sdf.grad of the chain's ops (the row chain runs it itself; the packed chain's packed_diff is differentiable once, so
    the restatement alone is the reference there)"""
    if layout == "packed":
        sdf, pi, app, g = _pack_case("noisy", 0, "gaps")
    else:
        (sdf, g), pi, app = _row_case("noisy", 0, 65), None, None
    inv_s = 20.0

    def second_order(alpha_of, x, s, g_out):
        alpha = alpha_of(x, s)
        gx, gs = torch.autograd.grad(alpha, (x, s), g_out.to(alpha.dtype) if alpha.shape == g_out.shape else g_out[..., :-1].to(alpha.dtype),
                                     create_graph=True)
        ((gx * gx).sum() + gs * gs).backward()
        return alpha, x.grad

    got = {}
    for fused in (True, False) if layout == "rows" else (True,):
        with _switch(fused) as nu:
            a = app.clone().requires_grad_(True) if mode == "sdf" else None
            call = ((lambda x, s: nu.neus_ray_sdf_to_alpha(x, s, append_cdf_1=mode == "one")) if pi is None else
                    (lambda x, s: nu.neus_packed_sdf_to_alpha(x, s, pi, append_cdf_1=mode == "one", pack_sdf_appends=a)))
            alpha, got[fused] = second_order(call, sdf.detach().clone().requires_grad_(True), torch.tensor(inv_s, device=dev, requires_grad=True), g)
            assert (type(alpha.grad_fn).__name__ == FUSED_NODE) == fused
    # float64 and fp32 of the same second-order expression through the restatement's ops
    refs = []
    pinfo = pi if pi is not None else ref.row_pack_infos(sdf.shape[0], sdf.shape[1], dev)
    nxt, valid = ref._next_index(pinfo, sdf.numel(), mode != "none")
    for dtype in (torch.float64, torch.float32):
        def restated(x, s):
            cdf = torch.sigmoid(x.reshape(-1) * s)
            P = pinfo.shape[0]
            tail = cdf.new_ones(P) if mode == "one" else (torch.sigmoid(app.to(dtype) * s) if mode == "sdf" else cdf.new_zeros(P))
            alpha = (torch.where(valid, -(torch.cat([cdf, tail])[nxt] - cdf), torch.zeros_like(cdf)) / (cdf + 1e-5)).clamp_min(0)
            if pi is None:
                alpha = alpha.reshape(sdf.shape)
                return alpha if mode == "one" else alpha[:, :-1]
            return alpha
        refs.append(second_order(restated, sdf.detach().clone().to(dtype).requires_grad_(True), torch.tensor(inv_s, device=dev, dtype=dtype, requires_grad=True),
                                 g)[1])
    for fused, grad in got.items():
        _check(f"create_graph {layout} append {mode} {'fused' if fused else 'chain'} second-order sdf.grad", grad, refs[0], refs[1])


def test_nan(dev):
    """one NaN in sdf: NaN at the same alpha positions as the chain wherever the sample closes an interval or is the c_next of one,
    finite values elsewhere.  Where there is no interval -- the last sample of a pack without append, a row outside every pack -- the
    kernel does not read the sample and gives the 0 of the issue's table; the chain divides its 0 by sigmoid(NaN) + 1e-5 and gives NaN."""
    sdf, pi, app, g = _pack_case("noisy", 0, "gaps")
    sdf = sdf.clone()
    b, n = pi[9].tolist()
    sdf[b + 70] = float("nan")
    rows = _row_case("noisy", 0, 65)[0].clone()
    rows[3, 64], rows[5, 0] = float("nan"), float("nan")
    with torch.no_grad(), _switch(True) as nu:
        for append in (False, True):
            on, off = nu.neus_packed_sdf_to_alpha(sdf, 256.0, pi, append), nu.neus_packed_sdf_to_alpha(sdf, 256.0, pi, append, fused=False)
            assert torch.equal(on.isnan(), off.isnan()) and int(on.isnan().sum()) == 2 and bool(on[~on.isnan()].isfinite().all())
            on, off = nu.neus_ray_sdf_to_alpha(rows, 256.0, append), nu.neus_ray_sdf_to_alpha(rows, 256.0, append, fused=False)
            assert torch.equal(on.isnan(), off.isnan()) and int(on.isnan().sum()) == (3 if append else 2)
            assert bool(on[~on.isnan()].isfinite().all())
        # no interval: a NaN on a pack's last sample (mode none) and on a row outside every pack, ordered and unordered packs
        for layout in ("gaps", "shuffled"):
            sdf, pi, app, g = _pack_case("noisy", 0, layout)
            sdf = sdf.clone()
            b, n = [(b, n) for b, n in pi.tolist() if n == 200][0]
            gap = int(_outside(pi, sdf.numel(), dev).nonzero()[0])
            sdf[b + n - 1], sdf[gap] = float("nan"), float("nan")
            on, off = nu.neus_packed_sdf_to_alpha(sdf, 256.0, pi), nu.neus_packed_sdf_to_alpha(sdf, 256.0, pi, fused=False)
            assert on.isnan().nonzero().flatten().tolist() == [b + n - 2]          # the interval whose c_next is the NaN
            assert float(on[b + n - 1]) == 0.0 and float(on[gap]) == 0.0
            assert sorted(off.isnan().nonzero().flatten().tolist()) == sorted([b + n - 2, b + n - 1, gap])
            assert torch.equal(on[~off.isnan()], off[~off.isnan()]) or bool(((on - off)[~off.isnan()].abs() <= 1e-5).all())
            one = nu.neus_packed_sdf_to_alpha(sdf, 256.0, pi, True)                # with an append the last sample closes an interval
            assert sorted(one.isnan().nonzero().flatten().tolist()) == [b + n - 2, b + n - 1]


# ---- the drivers: a scene as in tests/test_neus_query_gpu.py, with a learnable inv_s ------------------------------------------------
class SphereSDF(torch.nn.Module):
    """analytic model: sdf = |x| - r; colour = position-dependent; the protocol of the NeuS driver.  Keeps the SDF of the last
    differentiable query so that the test can read dL/dsdf per sample."""
    use_view_dirs = True

    def __init__(self, accel, dev, radius=0.62, inv_s=48.0):
        super().__init__()
        self.accel = accel
        self.radius = torch.nn.Parameter(torch.tensor(radius, device=dev))
        self.inv_s = torch.nn.Parameter(torch.tensor(inv_s, device=dev))
        self.last_sdf = None

    def forward_inv_s(self):
        return self.inv_s

    def forward_sdf(self, x, **kw):
        sdf = x.norm(dim=-1) - self.radius
        if sdf.requires_grad:
            sdf.retain_grad()
            self.last_sdf = sdf
        return dict(sdf=sdf)

    def forward(self, x, v=None, nablas_has_grad=False, with_rgb=True, with_normal=True, **kw):
        out = dict(sdf=x.norm(dim=-1) - self.radius)
        if with_normal:
            out["nablas"] = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-10)
        if with_rgb:
            out["rgb"] = torch.sigmoid(x + (v if v is not None else 0))
        return out


def _scene(dev, side=12, res=32):
    from demo_field import StaticOccGridAccel, pinhole_rays
    c = (np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1) + 0.5) / res * 2 - 1
    r = np.linalg.norm(c, axis=-1)
    occ = (r > 0.45) & (r < 0.8)
    model = SphereSDF(StaticOccGridAccel(torch.from_numpy(occ).to(dev), 0.03, max_steps=128), dev).train()
    o, d, near, far = pinhole_rays(side, dev, fov=0.25)
    n = side * side
    return model, dict(num_rays=n, rays_o=o, rays_d=d, near=near, far=far, rays_inds=torch.arange(n, device=dev))


def _sample_keys(vb):
    """one int64 per kept sample: (ray, bits of t) -- the depths come from the no-grad up-sampling and are the same on both routes"""
    rays = torch.repeat_interleave(vb["rays_inds_hit"], vb["pack_infos_hit"][:, 1])
    return (rays << 32) | (vb["t"].contiguous().view(torch.int32).long() & 0xFFFFFFFF)


def _driver_run(dev, fused, kw, monkeypatch):
    """one training-mode query and backward of sum(opacity_alpha), with what the opacity step saw recorded: its sdf (the model keeps
    it), its alpha before compression and dL/dalpha there (the compression is wrapped), and the packs"""
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    model, rays = _scene(dev)
    seen = {}
    real = rq.packed_volume_render_compression

    def recording(alpha, pack_infos, *a, **k):
        alpha.retain_grad()
        seen.update(alpha=alpha, pack_infos=pack_infos)
        return real(alpha, pack_infos, *a, **k)

    monkeypatch.setattr(rq, "packed_volume_render_compression", recording)
    with _switch(fused):
        vb, _ = rq.neus_ray_query_march_occ_multi_upsample_compressed(model, rays, **kw)
    monkeypatch.setattr(rq, "packed_volume_render_compression", real)
    assert vb["type"] == "packed" and vb["opacity_alpha"].grad_fn is not None
    vb["opacity_alpha"].sum().backward()
    sdf = model.last_sdf
    return dict(vb=vb, keys=_sample_keys(vb), sdf=sdf.detach(), g_sdf=sdf.grad, alpha=seen["alpha"].detach(), g=seen["alpha"].grad,
                pack_infos=seen["pack_infos"], g_radius=model.radius.grad, g_inv_s=model.inv_s.grad, inv_s=float(model.inv_s.detach()))


@pytest.mark.parametrize("num_coarse", [16, 0])
def test_compressed_driver_switch_on_against_off(dev, num_coarse, monkeypatch):
    """neus_ray_query_march_occ_multi_upsample_compressed in training mode with a learnable inv_s: packed final opacities with coarse
    samples, rows without.  Each route against the float64 evaluation of what its opacity step saw, and the two against each other."""
    kw = dict(num_coarse=num_coarse, num_fine=4, upsample_inv_s_factors=[1, 4], with_rgb=False, with_normal=False)
    on, off, again = (_driver_run(dev, fused, kw, monkeypatch) for fused in (True, False, False))
    assert torch.equal(off["keys"], again["keys"]) and torch.equal(off["vb"]["opacity_alpha"], again["vb"]["opacity_alpha"])
    assert torch.equal(on["sdf"], off["sdf"]) and torch.equal(on["pack_infos"], off["pack_infos"])    # the same input on both routes
    for name, r in (("on", on), ("off", off)):
        for k in ("g_radius", "g_inv_s"):
            assert r[k] is not None and bool(torch.isfinite(r[k])) and float(r[k].abs()) > 0
        rows = r["sdf"].dim() == 2
        g = torch.cat([r["g"].reshape(r["sdf"].shape[0], -1), r["g"].new_zeros(r["sdf"].shape[0], 1)], 1) if rows else r["g"]
        kwr = dict(pack_infos=None if rows else r["pack_infos"])
        print(f"driver num_coarse {num_coarse} switch {name}: {ref.near_ties(r['sdf'], r['inv_s'], **kwr)} intervals within 1e-4 of a tie")
        r64, r32 = (ref.chain(r["sdf"], r["inv_s"], g, dtype=d, **kwr) for d in (torch.float64, torch.float32))
        tag = f"driver num_coarse {num_coarse} switch {name}"
        _check(f"{tag} alpha before compression", r["alpha"].reshape(r64["alpha"].shape), r64["alpha"], r32["alpha"])
        _check(f"{tag} dL/dsdf", r["g_sdf"], r64["g_sdf"], r32["g_sdf"])
        _check_scalar(f"{tag} dL/dinv_s", r["g_inv_s"], r64, r32)
        # the radius: d sdf_i / d radius = -1, so its gradient is -sum_i dL/dsdf_i and T the sum of |dL/dsdf_i|
        want, T = -float(r64["g_sdf"].sum()), float(r64["g_sdf"].abs().sum())
        err, err32 = abs(float(r["g_radius"]) - want), abs(-float(r32["g_sdf"].sum()) - want)
        print(f"YARDSTICK {tag} dL/dradius: err {err:.3e} torch fp32 {err32:.3e} eps32 T {EPS32 * T:.3e} ratio {err / max(err32, EPS32 * T):.2f}")
        assert err <= 4 * max(err32, EPS32 * T)
    a_on, a_off = on["vb"]["opacity_alpha"].detach(), off["vb"]["opacity_alpha"].detach()
    if torch.equal(on["vb"]["pack_infos_hit"], off["vb"]["pack_infos_hit"]) and torch.equal(on["keys"], off["keys"]):
        assert torch.equal(on["vb"]["rays_inds_hit"], off["vb"]["rays_inds_hit"])
    else:
        # an alpha on the compaction's threshold: the routes keep different samples -- reported, capped, compared on the common ones
        common_on, common_off = torch.isin(on["keys"], off["keys"]), torch.isin(off["keys"], on["keys"])
        differ = int((~common_on).sum() + (~common_off).sum())
        print(f"COMPACTION differs in {differ} of {max(a_on.numel(), a_off.numel())} samples")
        assert differ <= 0.005 * max(a_on.numel(), a_off.numel())
        a_on, a_off = a_on[common_on], a_off[common_off]
    err = float((a_on.double() - a_off.double()).abs().max()) / float(a_off.abs().max())
    print(f"YARDSTICK driver num_coarse {num_coarse} opacity_alpha on against off: rel err {err:.3e}")
    assert err <= 1e-5
