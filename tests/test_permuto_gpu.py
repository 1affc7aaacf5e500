"""Permutohedral encoder on the GPU (csrc/permuto*.hip) against the float64 restatement of the reference (tests/permuto_ref.py):
forward, dL/dx, dL/dparam, the double backward, the options, batching, the autograd surface and an SDF step through the fused
decoder.  A point that landed in another simplex would show up as a row far off the restatement: such rows are counted, printed
and must be none."""
import numpy as np
import pytest
import torch

import permuto_ref as R
from util import assert_close

pytestmark = pytest.mark.gpu

HALF_TOL = 1e-3      # one rounding to half (the LoTD half tests' bound)


def _setup(D, nf, dtype, shifts, N, seed=0, L=None, hs=2 ** 12):
    from nr3d_lib_amd.bindings import _permuto as B
    g = torch.Generator().manual_seed(seed)
    L = L or len(nf)
    res = list(np.geomspace(4.0, 96.0, L))
    m = B.PermutoEncMeta(D, hs, res, nf)
    r = R.create_meta(D, hs, res, nf)
    x = torch.rand(N, D, generator=g)
    p = torch.randn(m.n_params, generator=g).to(dtype).float()        # values representable in the table dtype
    sh = (10.0 * torch.randn(L, D, generator=g)) if shifts else None
    return m, r, x, p, sh, g


def _rowcheck(name, got, want, rel):
    """max |err| per point relative to the column scale; count rows that fail (a different simplex) and print the count"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    scale = want.abs().amax(0).clamp(min=1e-30)
    bad = ((got - want).abs() > rel * scale).any(1)
    n_bad = int(bad.sum())
    print(f"{name}: {n_bad} of {got.shape[0]} points off the restatement")
    assert n_bad == 0, f"{name}: {n_bad} points differ (first {torch.nonzero(bad)[:5, 0].tolist()})"


CASES = [(2, [4, 2, 2]), (3, [4, 4, 2, 2, 2, 2, 2, 2]), (4, [4, 4]), (7, [2] * 8), (16, [4, 2, 2]), (32, [4, 4]), (64, [2, 2])]


@pytest.mark.parametrize("D,nf", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shifts", [False, True])
def test_fwd_bwd_against_restatement(dev, D, nf, dtype, shifts):
    from nr3d_lib_amd.bindings import _permuto as B
    N = 2048 if D <= 16 else 384
    m, r, x, p, sh, g = _setup(D, nf, dtype, shifts, N, seed=D)
    x64 = x.double().requires_grad_(True)
    p64 = p.double().requires_grad_(True)
    y_ref = R.encode(r, x, p64, shifts=sh, x64=x64)
    gy = torch.randn(y_ref.shape, generator=g).to(dtype).double()
    dx_ref, dp_ref = torch.autograd.grad(y_ref, [x64, p64], gy)
    xd, pd = x.to(dev), p.to(dtype).to(dev)
    shd = sh.to(dev) if sh is not None else None
    y = B.permuto_enc_fwd(m, xd, pd, shd)
    assert y.dtype == dtype and y.shape == (N, m.n_encoded_dims) and torch.isfinite(y).all()
    tol = HALF_TOL if dtype == torch.float16 else 1e-5
    _rowcheck(f"y D={D}", y, y_ref, tol)
    assert_close(y.float(), y_ref.detach().numpy(), rel=tol, name="y")
    dx, dp = B.permuto_enc_bwd(m, gy.to(dtype).to(dev), xd, pd, shd, None, None, None, None, None, True, True)
    assert dx.dtype == torch.float32 and dp.dtype == dtype
    assert_close(dx, dx_ref.numpy(), rel=1e-5 if dtype == torch.float32 else 2e-5, name="dL_dx")
    assert_close(dp.float(), dp_ref.numpy(), rel=tol, name="dL_dparam", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))
    # each half alone, and feature-major dL_dy
    gyd = gy.to(dtype).to(dev)
    dx2, dp2 = B.permuto_enc_bwd(m, gyd.t().contiguous().t(), xd, pd, shd, need_input_grad=True, need_param_grad=False)
    assert dp2 is None and torch.equal(dx2, dx)
    dx3, dp3 = B.permuto_enc_bwd(m, gyd, xd, pd, shd, need_input_grad=False, need_param_grad=True)
    assert dx3 is None
    assert_close(dp3.float(), dp_ref.numpy(), rel=tol, name="dL_dparam alone", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))


@pytest.mark.parametrize("D,nf", [(2, [4, 2]), (3, [4, 4, 2, 2]), (7, [2] * 4), (16, [4, 4]), (64, [2])])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_double_backward_against_restatement(dev, D, nf, dtype):
    from nr3d_lib_amd.bindings import _permuto as B
    N = 1024 if D <= 16 else 256
    m, r, x, p, sh, g = _setup(D, nf, dtype, True, N, seed=100 + D)
    x64 = x.double().requires_grad_(True)
    p64 = p.double().requires_grad_(True)
    gy64 = torch.randn(N, m.n_encoded_dims, generator=g).to(dtype).double().requires_grad_(True)
    ggx = torch.randn(N, D, generator=g)
    y = R.encode(r, x, p64, shifts=sh, x64=x64)
    nab, = torch.autograd.grad(y, x64, gy64, create_graph=True)
    ggy_ref, gp_ref = torch.autograd.grad((nab * ggx.double()).sum(), [gy64, p64])
    ddy, dp = B.permuto_enc_bwd_bwd_input(m, ggx.to(dev), gy64.detach().to(dtype).to(dev), x.to(dev), p.to(dtype).to(dev),
                                          sh.to(dev), need_dL_ddLdy=True, need_dL_dparams=True)
    tol = HALF_TOL if dtype == torch.float16 else 1e-5
    assert torch.isfinite(ddy).all() and ddy.dtype == dtype
    assert_close(ddy.float(), ggy_ref.numpy(), rel=tol, name="dL/d(dL_dy)")
    lv = dict(level_offsets=r["level_offsets"], n_params=r["n_params"])
    assert_close(dp.float(), gp_ref.numpy(), rel=tol, name="dL/dparam (2nd order)", levels=lv)
    a, b = B.permuto_enc_bwd_bwd_input(m, ggx.to(dev), gy64.detach().to(dtype).to(dev), x.to(dev), p.to(dtype).to(dev),
                                       sh.to(dev), need_dL_ddLdy=False, need_dL_dparams=True)
    assert a is None
    assert_close(b.float(), gp_ref.numpy(), rel=tol, name="dL/dparam alone", levels=lv)
    a, b = B.permuto_enc_bwd_bwd_input(m, ggx.to(dev), gy64.detach().to(dtype).to(dev), x.to(dev), p.to(dtype).to(dev),
                                       sh.to(dev), need_dL_ddLdy=True, need_dL_dparams=False)
    assert b is None and torch.equal(a, ddy)


def test_max_level_and_max_pos_dims(dev):
    from nr3d_lib_amd.bindings import _permuto as B
    m, r, x, p, sh, g = _setup(7, [2] * 6, torch.float32, True, 1500, seed=7)
    x64, p64 = x.double().requires_grad_(True), p.double().requires_grad_(True)
    y_ref = R.encode(r, x, p64, shifts=sh, max_level=2, x64=x64)
    gy = torch.randn(y_ref.shape, generator=g)
    dx_ref, dp_ref = torch.autograd.grad(y_ref, [x64, p64], gy.double())
    y = B.permuto_enc_fwd(m, x.to(dev), p.to(dev), sh.to(dev), max_level=2)
    assert (y[:, 6:] == 0).all()
    assert_close(y, y_ref.detach().numpy(), name="y max_level=2")
    dx, dp = B.permuto_enc_bwd(m, gy.to(dev), x.to(dev), p.to(dev), sh.to(dev), None, None, None, 2, 3, True, True)
    assert (dx[:, 3:] == 0).all()
    assert_close(dx[:, :3], dx_ref[:, :3].numpy(), name="dL_dx max_pos_dims=3")
    assert_close(dp, dp_ref.numpy(), name="dL_dparam max_level=2", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))
    assert (B.permuto_enc_fwd(m, x.to(dev), p.to(dev), max_level=-1) == 0).all()
    assert B.permuto_enc_bwd(m, gy.to(dev), x.to(dev), p.to(dev), max_level=-1, need_input_grad=True) == (None, None)


@pytest.mark.parametrize("mode", ["bidx", "offsets", "batched"])
def test_batching(dev, mode):
    from nr3d_lib_amd.bindings import _permuto as B
    B_, N = 3, 900
    m, r, x, p1, sh, g = _setup(3, [4, 2, 2], torch.float32, True, N, seed=11)
    p = torch.randn(B_ * m.n_params, generator=g)
    bidx = boffs = None
    bds = 0
    if mode == "bidx":
        bidx = torch.randint(-1, B_, (N,), generator=g)
    elif mode == "offsets":
        bidx = torch.randint(0, 2, (N,), generator=g)
        boffs = torch.tensor([2 * m.n_params, 0])
    else:
        bds = N // B_
    x64, p64 = x.double().requires_grad_(True), p.double().requires_grad_(True)
    y_ref = R.encode(r, x, p64, shifts=sh, bidx=bidx, boffs=boffs, bds=bds, x64=x64)
    gy = torch.randn(y_ref.shape, generator=g)
    dx_ref, dp_ref = torch.autograd.grad(y_ref, [x64, p64], gy.double())
    dv = lambda t: None if t is None else t.to(dev)   # noqa: E731
    y = B.permuto_enc_fwd(m, x.to(dev), p.to(dev), sh.to(dev), dv(bidx), dv(boffs), bds)
    assert_close(y, y_ref.detach().numpy(), name=f"y {mode}")
    if bidx is not None:
        assert (y[bidx.to(dev) < 0] == 0).all()
    dx, dp = B.permuto_enc_bwd(m, gy.to(dev), x.to(dev), p.to(dev), sh.to(dev), dv(bidx), dv(boffs), bds, None, None, True, True)
    assert_close(dx, dx_ref.numpy(), name=f"dL_dx {mode}")
    assert_close(dp, dp_ref.numpy(), name=f"dL_dparam {mode}", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))


def _impl(dev, dtype, D=3, shifts=True, pos_scale=1.0):
    from nr3d_lib_amd.models.grid_encodings.permuto import PermutoEncImpl
    torch.manual_seed(0)
    return PermutoEncImpl(D, [4., 9., 20., 44.], [2, 2, 4, 4], log2_hashmap_size=12, apply_random_shifts_per_level=shifts,
                          pos_scale=pos_scale, dtype=dtype, device=dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_impl_autograd_pos_scale_loss_scale(dev, dtype):
    """PermutoEncFunction / PermutoEncBwdInputFunction: pos_scale as a per-dimension tensor, loss_scale 128 for half"""
    enc = _impl(dev, dtype, D=4, pos_scale=torch.tensor([1.0, 0.5, 2.0, 0.25]))
    r = R.create_meta(4, 2 ** 12, [4., 9., 20., 44.], [2, 2, 4, 4])
    g = torch.Generator().manual_seed(3)
    x = torch.rand(700, 4, generator=g)
    p = (torch.randn(enc.n_params, generator=g) * 0.1).to(dtype).float()
    pp = p.to(dev).requires_grad_(True)
    xx = x.to(dev).requires_grad_(True)
    y = enc(xx, pp)
    gy = torch.randn(y.shape, generator=g).to(dtype)
    dx, dp = torch.autograd.grad(y, [xx, pp], gy.to(dev))
    ps = enc.pos_scale.cpu()
    xs = (x * ps)
    x64, p64 = xs.double().requires_grad_(True), p.double().requires_grad_(True)
    y_ref = R.encode(r, xs, p64, shifts=enc.level_random_shifts.cpu(), x64=x64)
    dxs_ref, dp_ref = torch.autograd.grad(y_ref, [x64, p64], gy.double())
    tol = HALF_TOL if dtype == torch.float16 else 1e-5
    assert_close(y.float(), y_ref.detach().numpy(), rel=tol, name="y")
    assert_close(dx, (dxs_ref * ps.double()).numpy(), rel=tol if dtype == torch.float16 else 1e-5, name="dL_dx")
    assert_close(dp, dp_ref.numpy(), rel=tol, name="dL_dparam", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))
    # nablas with create_graph, then a loss on them: dL/d(dL_dy) and dL/dparam of the second order
    gyr = gy.to(dev).float().requires_grad_(True)
    nab = enc.backward_dydx(gyr, xx.detach(), pp)
    gyl = gy.double().requires_grad_(True)
    x64b = xs.double().requires_grad_(True)
    p64b = p.double().requires_grad_(True)
    nab_ref, = torch.autograd.grad(R.encode(r, xs, p64b, shifts=enc.level_random_shifts.cpu(), x64=x64b), x64b, gyl, create_graph=True)
    nab_ref = nab_ref * ps.double()
    assert_close(nab, nab_ref.detach().numpy(), rel=tol if dtype == torch.float16 else 1e-5, name="nablas")
    w = torch.randn(nab.shape, generator=g)
    a, b = torch.autograd.grad((nab * w.to(dev)).sum(), [gyr, pp])
    ar, br = torch.autograd.grad((nab_ref * w.double()).sum(), [gyl, p64b])
    assert_close(a, ar.numpy(), rel=tol, name="dL/d(dL_dy)")
    assert_close(b, br.numpy(), rel=tol, name="dL/dparam 2nd", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))


def test_input_batched(dev):
    from nr3d_lib_amd.models.grid_encodings.permuto import permuto_enc_fwd, generate_meta
    m = generate_meta(3, [4., 9.], [2, 2], 512)
    r = R.create_meta(3, 512, [4., 9.], [2, 2])
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 50, 3, generator=g)
    p = torch.randn(2 * m.n_params, generator=g)
    y = permuto_enc_fwd(x.to(dev), p.to(dev), meta=m, input_batched=True)
    assert y.shape == (2, 50, 4)
    y_ref = R.encode(r, x.view(-1, 3), p.double(), bds=50)
    assert_close(y.reshape(-1, 4), y_ref.numpy(), name="input_batched")


def test_encoding_trains_and_eikonal(dev):
    """PermutoEncoding: gradients land in flattened_params; backward_dydx under create_graph; an eikonal loss's parameter
    gradient equals the restatement's"""
    from nr3d_lib_amd.models.grid_encodings.permuto import PermutoEncoding
    torch.manual_seed(1)
    enc = PermutoEncoding(3, permuto_cfg=dict(res_list=[4., 9., 20.], n_feats_list=[2, 2, 2], hashmap_size=2 ** 10),
                          space_cfg=dict(type='aabb', aabb=[[-1, -1, -1], [1, 1, 1]]), param_init_cfg={'type': 'normal', 'std': 0.1},
                          dtype=torch.float, device=dev)
    opt = torch.optim.Adam(enc.parameters(), lr=1e-2)
    x = torch.rand(512, 3, device=dev) * 2 - 1
    target = x.norm(dim=-1, keepdim=True)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (enc(x).sum(-1, keepdim=True) - target).square().mean()
        loss.backward()
        assert enc.flattened_params.grad is not None and enc.flattened_params.grad.abs().sum() > 0
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0]
    # eikonal on nablas = backward_dydx(ones)
    enc.zero_grad()
    xi = x[:200]
    gy = torch.ones(200, enc.out_features, device=dev)
    nab = enc.backward_dydx(gy, xi)
    loss = ((nab.norm(dim=-1) - 1) ** 2).mean()
    loss.backward()
    r = R.create_meta(3, 2 ** 10, [4., 9., 20.], [2, 2, 2])
    xs = (xi / 2 + 0.5).cpu()
    x64 = xs.double().requires_grad_(True)
    p64 = enc.flattened_params.detach().cpu().double().requires_grad_(True)
    y = R.encode(r, xs, p64, shifts=enc.permuto.level_random_shifts.cpu(), x64=x64)
    nab_ref, = torch.autograd.grad(y, x64, gy.cpu().double(), create_graph=True)
    loss_ref = (((nab_ref / 2).norm(dim=-1) - 1) ** 2).mean()
    gp, = torch.autograd.grad(loss_ref, p64)
    assert_close(enc.flattened_params.grad, gp.numpy(), name="eikonal dL/dparam", levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))
    assert set(enc.stat_param(with_grad=True)) >= {"grad.lv.0.norm", "lv.2.mean"}


def test_sdf_step_through_fused_decoder(dev):
    """PermutoEncoding -> fused MLP(.., D=1, W=64): nablas from the decoder's create_graph backward and backward_dydx, eikonal +
    SDF loss; lattice and decoder gradients against the same step on the restatement with a torch MLP"""
    from nr3d_lib_amd.models.blocks import MLP
    from nr3d_lib_amd.models.grid_encodings.permuto import PermutoEncoding
    torch.manual_seed(2)
    res, nf = [4., 8., 16., 32.], [2, 2, 2, 2]
    enc = PermutoEncoding(3, permuto_cfg=dict(res_list=res, n_feats_list=nf, hashmap_size=2 ** 11),
                          param_init_cfg={'type': 'normal', 'std': 0.5}, dtype=torch.float, device=dev)
    dec = MLP(enc.out_features, 1, D=1, W=64, dtype=torch.float, device=dev)
    x = torch.rand(1000, 3, device=dev)
    h = enc(x)
    sdf = dec(h)[..., 0]
    dL_dh, = torch.autograd.grad(sdf, h, torch.ones_like(sdf), create_graph=True)
    assert type(dL_dh.grad_fn).__name__ == "FusedMLPBackwardFunctionBackward"
    nab = enc.backward_dydx(dL_dh, x)
    loss = ((nab.norm(dim=-1) - 1) ** 2).mean() + sdf.abs().mean()
    loss.backward()
    # restatement + torch MLP (same weights) in float64
    r = R.create_meta(3, 2 ** 11, res, nf)
    lin = [mm for mm in dec.modules() if isinstance(mm, torch.nn.Linear) or hasattr(mm, "weight") and mm.weight.dim() == 2]
    ws = [mm.weight.detach().cpu().double().requires_grad_(True) for mm in lin]
    bs = [mm.bias.detach().cpu().double().requires_grad_(True) for mm in lin]
    assert len(ws) == 2
    p64 = enc.flattened_params.detach().cpu().double().requires_grad_(True)
    xc = x.cpu()
    x64 = xc.double().requires_grad_(True)
    hr = R.encode(r, xc, p64, shifts=enc.permuto.level_random_shifts.cpu(), x64=x64)
    hr_ = hr.detach().requires_grad_(True)
    sd = (torch.relu(hr_ @ ws[0].t() + bs[0]) @ ws[1].t() + bs[1])[:, 0]
    dh, = torch.autograd.grad(sd, hr_, torch.ones_like(sd), create_graph=True)
    nab_r, = torch.autograd.grad(hr, x64, dh, create_graph=True)
    sd_full = (torch.relu(hr @ ws[0].t() + bs[0]) @ ws[1].t() + bs[1])[:, 0]
    loss_r = ((nab_r.norm(dim=-1) - 1) ** 2).mean() + sd_full.abs().mean()
    gp, gw0, gw1 = torch.autograd.grad(loss_r, [p64, ws[0], ws[1]])
    assert_close(enc.flattened_params.grad, gp.numpy(), rel=1e-4, name="lattice grad",
                 levels=dict(level_offsets=r["level_offsets"], n_params=r["n_params"]))
    assert_close(lin[0].weight.grad, gw0.numpy(), rel=1e-4, name="decoder W0 grad")
    assert_close(lin[1].weight.grad, gw1.numpy(), rel=1e-4, name="decoder W1 grad")


def test_full_size_reference_workload(dev):
    """3,653,653 points, 7-D, 8 levels of 2 features, 16..2048, 2^16 tables, half: finite, every row written, an 8192-point
    subsample against the restatement"""
    from nr3d_lib_amd.bindings import _permuto as B
    res = [16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0]
    m = B.PermutoEncMeta(7, 2 ** 16, res, [2] * 8)
    r = R.create_meta(7, 2 ** 16, res, [2] * 8)
    N = 3653653
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(N, 7, device=dev, generator=g)
    p = torch.randn(m.n_params, device=dev, generator=g).half()
    y = B.permuto_enc_fwd(m, x, p)
    assert torch.isfinite(y).all()
    gy = torch.randn(N, 16, device=dev, generator=g).half()
    dx, dp = B.permuto_enc_bwd(m, gy, x, p, need_input_grad=True, need_param_grad=True)
    assert torch.isfinite(dx).all() and torch.isfinite(dp).all()
    ggx = torch.randn(N, 7, device=dev, generator=g)
    ddy, dp2 = B.permuto_enc_bwd_bwd_input(m, ggx, gy, x, p, need_dL_ddLdy=True, need_dL_dparams=True)
    assert torch.isfinite(ddy).all() and torch.isfinite(dp2).all()
    sel = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:8192]
    xs = x[sel.to(dev)].cpu()
    x64 = xs.double().requires_grad_(True)
    y_ref = R.encode(r, xs, p.cpu().double(), x64=x64)
    _rowcheck("full-size y", y[sel.to(dev)].float(), y_ref, HALF_TOL)
    dx_ref, = torch.autograd.grad(y_ref, x64, gy[sel.to(dev)].cpu().double(), create_graph=True)
    assert_close(dx[sel.to(dev)], dx_ref.detach().numpy(), rel=2e-5, name="full-size dL_dx subsample")
    # dL/d(dL_dy) of the double backward on the same rows: (dL_dx . ggx) differentiated by dL_dy
    gy64 = gy[sel.to(dev)].cpu().double().requires_grad_(True)
    x64b = xs.double().requires_grad_(True)
    nab, = torch.autograd.grad(R.encode(r, xs, p.cpu().double(), x64=x64b), x64b, gy64, create_graph=True)
    ddy_ref, = torch.autograd.grad((nab * ggx[sel.to(dev)].cpu().double()).sum(), gy64)
    _rowcheck("full-size dL/d(dL_dy)", ddy[sel.to(dev)].float(), ddy_ref, HALF_TOL)
    # the two parameter gradients at full size against the same kernels over chunks of 2^20 points (any index that went wrong only
    # at large N would differ), on an fp32 copy of the table (the gradients do not read it); the half results as that, rounded
    lv = dict(level_offsets=r["level_offsets"], n_params=r["n_params"])
    pf = p.float()
    _, dpf = B.permuto_enc_bwd(m, gy.float(), x, pf, need_input_grad=False, need_param_grad=True)
    _, dp2f = B.permuto_enc_bwd_bwd_input(m, ggx, gy.float(), x, pf, need_dL_ddLdy=False, need_dL_dparams=True)
    acc1, acc2 = torch.zeros_like(dpf), torch.zeros_like(dpf)
    for a in range(0, N, 1 << 20):
        b = min(N, a + (1 << 20))
        acc1 += B.permuto_enc_bwd(m, gy[a:b].float(), x[a:b], pf, need_input_grad=False, need_param_grad=True)[1]
        acc2 += B.permuto_enc_bwd_bwd_input(m, ggx[a:b], gy[a:b].float(), x[a:b], pf, need_dL_ddLdy=False, need_dL_dparams=True)[1]
    assert_close(dpf, acc1.cpu().numpy(), rel=5e-5, name="full-size dL_dparam vs chunks", levels=lv)
    assert_close(dp2f, acc2.cpu().numpy(), rel=5e-5, name="full-size 2nd-order dL_dparam vs chunks", levels=lv)
    assert_close(dp.float(), dpf.cpu().numpy(), rel=HALF_TOL, name="full-size half dL_dparam", levels=lv)
    assert_close(dp2.float(), dp2f.cpu().numpy(), rel=HALF_TOL, name="full-size half 2nd-order dL_dparam", levels=lv)


class _NoLaunch:
    """stands in for the library: any entry point called means an argument check let a bad tensor through"""
    def __getattr__(self, name):
        def f(*a, **k):
            raise AssertionError(f"{name} was called with an argument the binding should have refused")
        return f


def test_arguments_refused_before_launch(dev, monkeypatch):
    """every tensor the kernels read must be on the positions' device, batch offsets aligned and inside the table, the table
    storage aligned: checked in Python before any launch (the library is replaced by a stub that fails when called)"""
    from nr3d_lib_amd.bindings import _permuto as B
    m = B.PermutoEncMeta(3, 256, [4., 8.], [2, 2])
    x = torch.rand(64, 3, device=dev)
    p = torch.randn(2 * m.n_params + 2, device=dev)
    p1 = p[:m.n_params]
    gy = torch.randn(64, m.n_encoded_dims, device=dev)
    ggx = torch.randn(64, 3, device=dev)
    bidx = torch.zeros(64, dtype=torch.long, device=dev)
    m._scales(dev)
    monkeypatch.setattr(B.H, "lib", lambda: _NoLaunch())
    bad = [
        lambda: B.permuto_enc_fwd(m, x, p1, batch_inds=bidx.cpu()),
        lambda: B.permuto_enc_fwd(m, x, p1, batch_inds=bidx, batch_offsets=torch.tensor([0])),
        lambda: B.permuto_enc_bwd(m, gy.cpu(), x, p1, need_input_grad=True, need_param_grad=True),
        lambda: B.permuto_enc_bwd(m, gy, x, p1, batch_inds=bidx.cpu(), need_input_grad=True),
        lambda: B.permuto_enc_bwd_bwd_input(m, ggx.cpu(), gy, x, p1, need_dL_ddLdy=True, need_dL_dparams=True),
        lambda: B.permuto_enc_bwd_bwd_input(m, ggx, gy.cpu(), x, p1, need_dL_ddLdy=True, need_dL_dparams=True),
        lambda: B.permuto_enc_bwd_bwd_input(m, ggx, gy, x, p1, batch_offsets=torch.tensor([0]), batch_inds=bidx,
                                            need_dL_dparams=True),
        # misaligned / out-of-range batch offsets, misaligned table storage, more batches than table sets
        lambda: B.permuto_enc_fwd(m, x, p[:2 * m.n_params], batch_inds=bidx, batch_offsets=torch.tensor([1], device=dev)),
        lambda: B.permuto_enc_fwd(m, x, p[:2 * m.n_params], batch_inds=bidx, batch_offsets=torch.tensor([m.n_params + 2], device=dev)),
        lambda: B.permuto_enc_fwd(m, x, p[:2 * m.n_params], batch_inds=bidx, batch_offsets=torch.tensor([-2], device=dev)),
        lambda: B.permuto_enc_fwd(m, x, p[1:1 + m.n_params]),
        lambda: B.permuto_enc_fwd(m, x, p1, batch_data_size=32),
    ]
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda:1")
        bad += [lambda: B.permuto_enc_fwd(m, x, p1, batch_inds=bidx.to(other)),
                lambda: B.permuto_enc_bwd(m, gy.to(other), x, p1, need_input_grad=True)]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
